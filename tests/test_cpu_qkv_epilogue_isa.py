"""The epilogue operands of the conv_dma kernels, counted in the gfx950 code of the built library (extracted and disassembled as
tests/test_cpu_prologue_isa.py does; its `kernels` fixture and selection are used here).

What is held, in EVERY conv_dma kernel outside the vocoder's (VOC) and the GroupNorm fold's (GNF), conv_dma_pair_kernel included:
  * the per-row constants of the epilogue (bias; the LayerNorm fold's ln_c1 / ln_c2) arrive as 16-byte loads -- register buffer loads in
    single-tile kernels (late_loads), global_load_dwordx4 in the others (row_consts): no plain 4-byte global load is left but the
    one or two of the column statistics' set-up.  The cluster join's partial tiles are 4-byte loads by design (one register of 64
    lanes = one 256-byte line) and are told apart by their sc1 bit;
  * 64-bit vector address arithmetic (v_lshl_add_u64) is below the parent build's in every kernel;
  * 4-byte global stores are NOT above the parent build's in any kernel.  They are not below it either: the sixteen of the value rows'
    VT path (store_vt) are still there.  The 16-byte form that removed them from the 1x1 64 x 64 kernel (65 -> 49) was measured inside
    the A/B's spread and taken out again, so the count that was to fall by sixteen stands where it stood.

Counts of the parent build -> of this build, per class of kernel (the same in every instantiation of a class):
    32-row tiles per wave, kernel     kernels   global_load_dword (no sc1)   global_store_dword   v_lshl_add_u64   global_load_dwordx4
    1, k 1 (32 x 64, 64 x 64)            17            1 -> 1                    65 -> 65            93 -> 91            8 -> 8
    1, k 2 / k 3 / fused pair            25            1 -> 0                    65 -> 65            93 -> 71            8 -> 0
    2, k 1 (128 x 64)                    10           65 -> 1                   129 -> 129          240 -> 179           0 -> 16
    2, k 3                                3           65 -> 0                   129 -> 129          240 -> 156           0 -> 8
    4, k 1 (128 x 128)                    7           66 -> 2                   192 -> 192          414 -> 353           0 -> 16
    4, k 3                                3           66 -> 0                   192 -> 192          414 -> 310           0 -> 8
(The parent's single-tile kernels already held their fold constants as eight dwordx4 loads: the compiler had merged the 32 contiguous rows.
They stood at the top of the epilogue; in a 1x1 kernel they are late loads now and the eight that are left belong to a fold with a
residual, and the other kernels have no fold at all.)

Bounds: loads and address adds at this build's count plus a slack of 2 and 8, room for the compiler's scheduling and none for a path
coming back (a 4-byte constants path is 16 loads per tile row and array; the address adds must also stay below the parent's); stores at
the parent's count, no slack."""
import re

import pytest

from test_cpu_prologue_isa import checked, kernels, template_args  # noqa: F401  (kernels: the module-scoped fixture)

# (32-row tiles per wave, 1x1 kernel): (plain 4-byte loads, 4-byte stores, 64-bit address adds) of the parent build / of this build
PARENT = {(1, True): (1, 65, 93), (1, False): (1, 65, 93), (2, True): (65, 129, 240), (2, False): (65, 129, 240), (4, True): (66, 192, 414), (4, False): (66, 192, 414)}
BUILT = {(1, True): (1, 65, 91), (1, False): (0, 65, 71), (2, True): (1, 129, 179), (2, False): (0, 129, 156), (4, True): (2, 192, 353), (4, False): (0, 192, 310)}
SLACK_LOAD4, SLACK_ADD64 = 2, 8


def count(body, pat):
    return sum(re.match(pat, ins) is not None for ins in body)


def classes(kernels):
    """[(template arguments, class, body)] of every checked kernel"""
    out = []
    for name, body in checked(kernels).items():
        a = template_args(name)
        if "conv_dma_pair_kernel" in name:
            cls = (1, False)
        else:
            cls = (max(1, a[0] * a[1] // (64 * 64)), a[2] == 1)
        assert cls in PARENT, (a, cls)
        out.append((a, cls, body))
    assert len(out) >= 60, len(out)
    return out


def test_no_4_byte_constant_loads(kernels):
    bad = []
    for a, cls, body in classes(kernels):
        n = sum(re.match(r"^global_load_dword\s", ins) is not None and "sc1" not in ins for ins in body)
        if n > BUILT[cls][0] + SLACK_LOAD4:
            bad.append((a, n))
    assert not bad, f"(template arguments, plain 4-byte global loads): {bad}"


def test_row_constants_are_16_byte_global_loads_in_multi_tile_kernels(kernels):
    """1x1 kernels of two or four tiles per wave: 4 quads x 2 arrays x 2 tile rows (the fold)"""
    bad = []
    for a, cls, body in classes(kernels):
        if cls[0] >= 2 and cls[1]:
            x4 = count(body, r"^global_load_dwordx4\s")
            if x4 < 16:
                bad.append((a, x4))
    assert not bad, f"(template arguments, global_load_dwordx4): {bad}"


def test_4_byte_stores_not_above_the_parent(kernels):
    bad = []
    for a, cls, body in classes(kernels):
        st4 = count(body, r"^global_store_dword\s")
        if st4 > PARENT[cls][1]:
            bad.append((a, st4, PARENT[cls][1]))
    assert not bad, f"(template arguments, 4-byte global stores, the parent's): {bad}"


def test_64_bit_address_arithmetic_below_the_parent(kernels):
    bad = []
    for a, cls, body in classes(kernels):
        n = count(body, r"^v_lshl_add_u64\s")
        if n >= PARENT[cls][2] or n > BUILT[cls][2] + SLACK_ADD64:
            bad.append((a, n, PARENT[cls][2]))
    assert not bad, f"(template arguments, v_lshl_add_u64, the parent's): {bad}"
