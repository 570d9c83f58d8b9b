"""What the conv_dma kernels do before their first operand DMA, and the form of their K4P stores, read from the gfx950 code in the built
library (extracted the way test_cpu_no_spills.py does, then disassembled); and the launchers' division-free block-index decomposition
against plain / and %.

A UNet step pays the launch prologue some 12,000 times, so for every instantiation of conv_dma_kernel and conv_dma_pair_kernel outside
the vocoder's (VOC) and the GroupNorm fold's (GNF, which requests its statistics first on purpose), nothing that the first
`buffer_load ... lds` does not need may stand in front of it:
  * no vector load to registers (the epilogue's operands are requested behind the first tiles);
  * no v_rcp_iflag_f32 (the block index is decomposed on the scalar unit, csrc/kernels.h dma_magic);
  * at most 5 `s_waitcnt lgkmcnt(0)` and at most 100 vector-ALU instructions -- what the multi-tile instantiations, which never had
    epilogue loads in front, needed before this was checked (4-5 waits, 57-91 instructions).
The K4P output leaves as 16-byte stores (csrc/k4p.h k4p_tile_entries): a dwordx4 store in every kernel, no write-through dwordx2 store.
The counted waits behind the first burst are held to the code they count (test_counted_waits_match_the_late_loads)."""
import ctypes as ct
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

LLVM = "/opt/rocm/lib/llvm/bin"
LIB = os.path.join(ROOT, "latent-diffusion-speech_amd", "lds", "liblds.so")
OBJDUMP = os.path.join(LLVM, "llvm-objdump")

MAX_WAITS, MAX_VALU = 5, 100


def template_args(mangled):
    m = re.search(r"conv_dma(?:_pair)?_kernelI((?:L[ib]\d+E)+)E", mangled)
    return [int(v) for v in re.findall(r"L[ib](\d+)E", m.group(1))]


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{mangled name: [instruction lines]} of every conv_dma kernel in the library"""
    if not os.path.exists(OBJDUMP):
        pytest.skip("ROCm LLVM tools not installed")
    assert os.path.exists(LIB), "build the library first (__graft_entry__.build())"
    tmp = tmp_path_factory.mktemp("isa")
    lib = tmp / "liblds.so"
    shutil.copy(LIB, lib)
    subprocess.run([OBJDUMP, "--offloading", str(lib)], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=tmp)
    out = {}
    for f in sorted(os.listdir(tmp)):
        if "gfx950" not in f:
            continue
        syms = subprocess.run([OBJDUMP, "-t", str(tmp / f)], check=True, stdout=subprocess.PIPE, text=True).stdout
        if "conv_dma_kernel" not in syms and "conv_dma_pair_kernel" not in syms:
            continue
        dis = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", str(tmp / f)], check=True, stdout=subprocess.PIPE, text=True).stdout
        name = None
        for ln in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", ln)
            if m:
                name = m.group(1) if re.search(r"conv_dma(_pair)?_kernelI", m.group(1)) else None
                if name:
                    out[name] = []
                continue
            if name and ln.strip():
                out[name].append(ln.split("//")[0].strip())
    assert out, "no conv_dma kernel found in the library"
    return out


def checked(kernels):
    """the instantiations the bounds apply to: conv_dma_pair_kernel, and conv_dma_kernel without VOC (argument 8) and GNF (argument 9)"""
    sel = {}
    for name, body in kernels.items():
        a = template_args(name)
        if "conv_dma_pair_kernel" in name or (not a[8] and not a[9]):
            sel[name] = body
    assert len(sel) >= 40, len(sel)
    return sel


def is_lds_dma(ins):
    return re.match(r"^buffer_load_\w+ .*\blds\b", ins) is not None


def test_prologue_before_first_dma(kernels):
    bad = []
    for name, body in checked(kernels).items():
        first = next((i for i, ins in enumerate(body) if is_lds_dma(ins)), None)
        assert first is not None, f"{name}: no LDS-DMA load"
        pre = body[:first]
        ops = [ins.split()[0] for ins in pre]
        vloads = [ins for ins in pre if re.match(r"^(global|buffer|flat|scratch)_load", ins)]
        rcp = sum(op.startswith("v_rcp_iflag_f32") for op in ops)
        waits = sum(ins.startswith("s_waitcnt") and "lgkmcnt(0)" in ins for ins in pre)
        valu = sum(op.startswith("v_") for op in ops)
        if vloads or rcp or waits > MAX_WAITS or valu > MAX_VALU:
            bad.append((template_args(name), dict(vector_loads=len(vloads), rcp=rcp, waits=waits, valu=valu)))
    assert not bad, f"work in front of the first DMA: {bad}"


def test_k4p_stores_are_16_bytes(kernels):
    bad = []
    for name, body in checked(kernels).items():
        x4 = sum(re.match(r"^(global|buffer)_store_dwordx4\b", ins) is not None for ins in body)
        x2wt = sum(re.match(r"^global_store_dwordx2\b.*\bsc1\b", ins) is not None for ins in body)
        x4wt = sum(re.match(r"^(global|buffer)_store_dwordx4\b.*\bsc1\b", ins) is not None for ins in body)
        swaps = sum(ins.startswith("v_permlane32_swap") for ins in body)
        # two swaps build one entry: fewer means that entries were put together from the same registers
        if x4 == 0 or x2wt or swaps < 2 * x4wt:
            bad.append((template_args(name), x4, x2wt, swaps, x4wt))
    assert not bad, f"(template arguments, dwordx4 stores, write-through dwordx2 stores, swaps, write-through dwordx4 stores): {bad}"


NLATE = 12      # csrc/conv_dma.hip late_loads(): 8 residual entries and 4 bias quads, as buffer loads to registers


def is_reg_buffer_load(ins):
    return ins.startswith("buffer_load_") and not is_lds_dma(ins)


def is_back_branch(ins):
    m = re.match(r"^s_c?branch\w*\s+(\d+)", ins)
    return m is not None and int(m.group(1)) >= 0x8000      # (a 16-bit signed offset printed unsigned)


def test_counted_waits_match_the_late_loads(kernels):
    """The counted waits of csrc/conv_dma.hip wait_younger allow NLATE more operations in flight while the awaited tile belongs to the first
    burst, which is only right if the code really holds NLATE vector memory operations between that burst and the wait: had the compiler
    dropped or moved one (an epilogue operand that became dead in some instantiation), the count would be too large and the first MFMAs
    would read LDS before the DMA has landed.  So, in every kernel that has the late loads (register buffer loads exist nowhere else in
    these kernels): between the last LDS-DMA of the burst in front of them and the next s_barrier stand exactly NLATE register buffer
    loads and no LDS-DMA, and the wait ladder in front of that barrier counts y * PER_TILE + NLATE for y = 0 .. NST - 1, with PER_TILE
    taken from the burst itself."""
    bad, seen = [], 0
    for name, body in checked(kernels).items():
        a = template_args(name)
        pair = "conv_dma_pair_kernel" in name
        nst = a[4] if pair else a[6]
        single = pair or (a[0] * a[1] <= 64 * 64)      # one 32 x 32 tile per wave: the instantiations that take the late loads
        L = next((i for i, ins in enumerate(body) if is_reg_buffer_load(ins)), None)
        if L is None:
            if single:
                bad.append((a, "no late loads in a single-tile instantiation"))
            continue
        seen += 1
        start = max([i for i in range(L) if body[i].startswith("s_barrier")], default=-1) + 1
        burst = [i for i in range(start, L) if is_lds_dma(body[i])]
        if not burst:
            bad.append((a, "no DMA burst in front of the late loads"))
            continue
        looped = any(is_back_branch(body[i]) for i in range(burst[0], L))
        per_tile, rem = (len(burst), 0) if looped else divmod(len(burst), nst)
        end = next(i for i in range(L, len(body)) if body[i].startswith("s_barrier"))
        late = sum(is_reg_buffer_load(body[i]) for i in range(burst[-1], end))
        dma_between = sum(is_lds_dma(body[i]) for i in range(burst[-1] + 1, end))
        # (a rung of the ladder is a compare, a branch and the wait: the window holds NST of them and nothing of ln_columns' own waits)
        ladder = [int(m.group(1)) for i in range(max(L, end - 6 * nst - 6), end) for m in [re.match(r"^s_waitcnt vmcnt\((\d+)\)", body[i])] if m]
        want = sorted({min(63, y * per_tile + NLATE) for y in range(nst)})
        if rem or late != NLATE or dma_between or not ladder or sorted(set(ladder)) != want:
            bad.append((a, dict(per_tile=per_tile, rem=rem, late_loads=late, dma_between=dma_between, ladder=ladder, want=want)))
    assert seen >= 10, seen
    assert not bad, f"late loads / counted waits: {bad}"


# ---- the block-index decomposition (host code: csrc/kernels.h dma_magic / dma_tile_of through include/lds_test.h) ----

# output rows of the UNet's convolutions (lds/arch.py unet_config: 80 mel bins, levels of 256 / 384 / 512 channels; QKV = 3 C, the feed-forward's
# GEGLU = 8 C and its inner width 4 C rows), and the widths of the tests' small layers
UNET_WIDTHS = (64, 80, 96, 128, 192, 256, 384, 512, 768, 1024, 1152, 1536, 2048, 3072, 4096)


def launcher_divisors(max_B=64, max_T=4096):
    """every divisor the launchers can pass for B <= 64, T <= 4096 and the UNet's channel widths (output rows padded to 64; FF1 has 8 C
    rows): M-blocks of 32 / 64 / 128 rows, frame blocks of 64 / 128 / 256 frames, cluster shares 1 .. 16"""
    nmb = {(-(-c // 64) * 64) // bm for c in UNET_WIDTHS for bm in (32, 64, 128) if (-(-c // 64) * 64) % bm == 0}
    nn = set(range(1, max_T // 64 + 1))
    return sorted(nmb | nn | {1, 2, 4, 8, 16}), max(nmb), max(nn)


def test_magic_division_exhaustive():
    from lds import native
    L = native.lib()
    divs, max_nmb, max_nn = launcher_divisors()
    n_count = max_nmb * max_nn * 64 + 8          # every block id (and intermediate quotient) of the largest grid: ksplit > 1 only shrinks it
    n = np.arange(n_count, dtype=np.uint32)
    out = np.empty(n_count, dtype=np.uint32)
    for d in divs:
        assert L.lds_test_dma_magic_div(d, n_count, out.ctypes.data_as(ct.c_void_p)) == 0
        assert np.array_equal(out, n // np.uint32(d)), d
    # the ends of the range the constants are exact for (n < 2^31, d < 2^31), in slices
    for d in (1, 2, 3, 7, 641, 65535, 65537, (1 << 31) - 1):
        cnt = 1 << 16
        o = np.empty(cnt, dtype=np.uint32)
        assert L.lds_test_dma_magic_div(d, cnt, o.ctypes.data_as(ct.c_void_p)) == 0
        assert np.array_equal(o, np.arange(cnt, dtype=np.uint32) // np.uint32(d)), d


@pytest.mark.parametrize("nMb,nN,B,S", [(1, 1, 1, 1), (2, 8, 16, 1), (5, 7, 3, 1), (20, 8, 16, 1), (40, 64, 64, 1), (3, 1, 1, 16), (10, 2, 2, 4), (80, 3, 5, 2),
                                        (6, 33, 7, 1), (1, 64, 64, 1)])
def test_tile_order_matches_division(nMb, nN, B, S):
    """the kernel's arithmetic with the launcher's constants gives the tile that / and % give: same id -> same (mb, nb, b, ksp)"""
    from lds import native
    total = nMb * nN * B * S
    out = np.empty((total, 4), dtype=np.int32)
    assert native.lib().lds_test_dma_tile_order(nMb, nN, B, S, out.ctypes.data_as(ct.c_void_p)) == 0
    idx = np.arange(total, dtype=np.int64)
    xcd, slot, per, rem = idx & 7, idx >> 3, total >> 3, total & 7
    Lin = xcd * per + np.minimum(xcd, rem) + slot
    mb, tb = Lin % nMb, Lin // nMb
    nb, by = tb % nN, tb // nN
    b, ksp = by // S, by % S
    assert np.array_equal(out, np.stack([mb, nb, b, ksp], axis=1).astype(np.int32))
    assert len({tuple(r) for r in out}) == total      # a permutation: every tile exactly once
