"""What attention_k4p_kernel does before its first K/V tile DMA and gn_stream_kernel before its first store, read from the gfx950 code in
the built library the way test_cpu_prologue_isa.py reads the conv_dma kernels (same extraction, other kernel names).

attention_k4p_kernel, every instantiation, in front of the first `buffer_load ... lds`:
  * no `s_waitcnt vmcnt` (the query fragments are requested unconditionally and waited for with tile 0);
  * no v_rcp_iflag_f32 (the block index is decomposed on the scalar unit, csrc/kernels.h dma_magic);
  * at most 2 `s_waitcnt lgkmcnt(0)` (the arguments in one burst; the ragged length);
  * fewer vector-ALU instructions than the parent build had, and at most this build's own count plus 10.
    <D, NW, NST, KS>           fp32: parent -> this build      split-fp16: parent -> this build
    <32,4,3,1> / <32,4,3,2>    109 / 108 -> 16 / 15            67 / 66 -> 16 / 15
    <32,1,2,1> / <32,4,9,4>     83 /  66 -> 32 / 15            71 / 66 -> 32 / 15
    <48,4,3,1> / <48,4,3,2>    173 / 172 -> 19 / 18           134 / 133 -> 19 / 18
    <48,1,2,1> / <48,4,5,4>    159 / 133 -> 44 / 18            97 / 133 -> 44 / 18
    <64,4,2,1> / <64,4,2,2>    208 / 207 -> 22 / 21            84 /  86 -> 22 / 21
    <64,1,2,1> / <64,4,4,4>    117 / 168 -> 56 / 21           141 /  90 -> 56 / 21
  (both builds with the Makefile's flags; the parent's waits in front of the DMA: 0-4 `vmcnt(0)`, 3 `lgkmcnt(0)`, 3 v_rcp_iflag_f32.)
The query loads are written in asm, which the compiler does not track: between each of them and the next `s_waitcnt vmcnt` nothing may
touch its destination registers (test_query_registers_rest_until_the_wait).

gn_stream_kernel<1|2|4>, in front of the first store: no v_rcp_iflag_f32 (parent: 2), at most 4 `s_waitcnt lgkmcnt(0)` (parent: 22, this
build: 2), `s_waitcnt vmcnt` not above the parent's 3 (this build: 3, one of them counted and two in the cold rounds' loops)."""
import os
import re
import shutil
import subprocess

import pytest

from test_cpu_prologue_isa import LIB, OBJDUMP, is_lds_dma

# (D, NW, NST, KS, F16) -> (the parent's VALU count in front of the first DMA, this build's)
ATT_VALU = {
    (32, 4, 3, 1, 0): (109, 16), (32, 4, 3, 2, 0): (108, 15), (32, 1, 2, 1, 0): (83, 32), (32, 4, 9, 4, 0): (66, 15),
    (48, 4, 3, 1, 0): (173, 19), (48, 4, 3, 2, 0): (172, 18), (48, 1, 2, 1, 0): (159, 44), (48, 4, 5, 4, 0): (133, 18),
    (64, 4, 2, 1, 0): (208, 22), (64, 4, 2, 2, 0): (207, 21), (64, 1, 2, 1, 0): (117, 56), (64, 4, 4, 4, 0): (168, 21),
    (32, 4, 3, 1, 1): (67, 16), (32, 4, 3, 2, 1): (66, 15), (32, 1, 2, 1, 1): (71, 32), (32, 4, 9, 4, 1): (66, 15),
    (48, 4, 3, 1, 1): (134, 19), (48, 4, 3, 2, 1): (133, 18), (48, 1, 2, 1, 1): (97, 44), (48, 4, 5, 4, 1): (133, 18),
    (64, 4, 2, 1, 1): (84, 22), (64, 4, 2, 2, 1): (86, 21), (64, 1, 2, 1, 1): (141, 56), (64, 4, 4, 4, 1): (90, 21),
}
GN_MAX_LGKM_WAITS, GN_MAX_VM_WAITS = 4, 3


def template_args(mangled):
    m = re.search(r"_kernelI((?:L[ib]\d+E)+)E", mangled)
    return tuple(int(v) for v in re.findall(r"L[ib](\d+)E", m.group(1)))


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{mangled name: [instruction lines]} of every attention_k4p_kernel and gn_stream_kernel in the library"""
    if not os.path.exists(OBJDUMP):
        pytest.skip("ROCm LLVM tools not installed")
    assert os.path.exists(LIB), "build the library first (__graft_entry__.build())"
    tmp = tmp_path_factory.mktemp("isa")
    lib = tmp / "liblds.so"
    shutil.copy(LIB, lib)
    subprocess.run([OBJDUMP, "--offloading", str(lib)], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=tmp)
    want = re.compile(r"attention_k4p_kernelI|gn_stream_kernelI")
    out = {}
    for f in sorted(os.listdir(tmp)):
        if "gfx950" not in f:
            continue
        syms = subprocess.run([OBJDUMP, "-t", str(tmp / f)], check=True, stdout=subprocess.PIPE, text=True).stdout
        if not want.search(syms):
            continue
        dis = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", str(tmp / f)], check=True, stdout=subprocess.PIPE, text=True).stdout
        name = None
        for ln in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", ln)
            if m:
                name = m.group(1) if want.search(m.group(1)) else None
                if name:
                    out[name] = []
                continue
            if name and ln.strip():
                out[name].append(ln.split("//")[0].strip())
    assert out, "no attention_k4p / gn_stream kernel found in the library"
    return out


def attention(kernels):
    sel = {template_args(n): b for n, b in kernels.items() if "attention_k4p_kernelI" in n}
    assert set(sel) == set(ATT_VALU), sorted(set(sel) ^ set(ATT_VALU))
    return sel


def counts(pre):
    ops = [ins.split()[0] for ins in pre]
    return dict(vm_waits=sum(ins.startswith("s_waitcnt") and "vmcnt" in ins for ins in pre),
                lgkm_waits=sum(ins.startswith("s_waitcnt") and "lgkmcnt(0)" in ins for ins in pre),
                rcp=sum(op.startswith("v_rcp_iflag_f32") for op in ops), valu=sum(op.startswith("v_") for op in ops))


def test_attention_prologue_before_first_dma(kernels):
    bad = []
    for a, body in attention(kernels).items():
        first = next((i for i, ins in enumerate(body) if is_lds_dma(ins)), None)
        assert first is not None, f"{a}: no LDS-DMA load"
        c = counts(body[:first])
        parent, own = ATT_VALU[a]
        if c["vm_waits"] or c["rcp"] or c["lgkm_waits"] > 2 or not c["valu"] < parent or c["valu"] > own + 10:
            bad.append((a, c, dict(parent_valu=parent, recorded_valu=own)))
    assert not bad, f"work in front of the first K/V DMA: {bad}"


def vregs(text):
    regs = set()
    for lo, hi in re.findall(r"\bv\[(\d+):(\d+)\]", text):
        regs.update(range(int(lo), int(hi) + 1))
    regs.update(int(r) for r in re.findall(r"\bv(\d+)\b", text))
    return regs


def test_query_registers_rest_until_the_wait(kernels):
    """every query fragment is one register buffer load (head dim / 8 of them) in front of the first DMA, and no instruction between a load and
    the next `s_waitcnt vmcnt` reads or writes its destination: the compiler takes the values as defined at the asm statement"""
    bad = []
    for a, body in attention(kernels).items():
        first = next(i for i, ins in enumerate(body) if is_lds_dma(ins))
        loads = [i for i in range(first) if body[i].startswith("buffer_load_dwordx4")]
        if len(loads) != a[0] // 8:
            bad.append((a, "query loads", len(loads)))
            continue
        wait = next(i for i in range(first, len(body)) if body[i].startswith("s_waitcnt") and "vmcnt" in body[i])
        for i in loads:
            dst = vregs(body[i].split(",")[0])
            touched = [body[j] for j in range(i + 1, wait) if vregs(body[j]) & dst]
            if touched:
                bad.append((a, body[i], touched[:3]))
    assert not bad, bad


def test_gn_stream_before_first_store(kernels):
    sel = {template_args(n): b for n, b in kernels.items() if "gn_stream_kernelI" in n}
    assert set(sel) == {(1,), (2,), (4,)}, sorted(sel)
    bad = []
    for a, body in sel.items():
        first = next(i for i, ins in enumerate(body) if re.match(r"^(buffer|global|flat|scratch)_store", ins))
        c = counts(body[:first])
        if c["rcp"] or c["lgkm_waits"] > GN_MAX_LGKM_WAITS or c["vm_waits"] > GN_MAX_VM_WAITS:
            bad.append((a, c))
    assert not bad, f"work in front of the first store: {bad}"
