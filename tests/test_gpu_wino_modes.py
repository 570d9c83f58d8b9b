"""gn_wino_kernel (csrc/k4p_ops.hip), conv_wino_kernel (csrc/conv_wino.hip) and their routing (csrc/model.hip wino_min_T, run_resnet) at the
widths, levels and routing edges that only whole-UNet runs reached: each kernel path below against a float64 numpy reference of the same
operation (tests/wino_numpy.py), through lds_test_wino_conv / lds_test_wino_conv_lvl.

Bounds: output against the float64 direct convolution relmax < 1e-5 (the per-kernel bound, tests/test_gpu_k4p.py); planes bit-equal to the
transform of lds_test_gn_apply's output on the same inputs (dense) or within 1e-5 of the float64 planes (ragged, as
tests/test_gpu_wino.py::test_wino_ragged_poisoned); that gn_apply output itself within 1e-5 of the float64 GroupNorm (test_gpu_k4p.py's
bound for it: the planes' bit-equality alone would pass a fault the two passes share, they have one prologue); epilogue partials 1e-5 / 1e-3
(check_partials of tests/test_gpu_wino.py).

Which group reaches what:
gn_wino_kernel
  * the E = 2 and E = 4 instantiations (T > 256, T > 512) and the second pass of the work loop (base > 0, T > 1024) ........ group a
  * the partials prologue beyond the first 64 partials of a group (second request; the loop from 128) ..................... group a
  * lvl > 0: the kernel reduces the level-0 lengths itself ................................................................ group f
  * the group-index magic division for the divisors 4 .. 16 (8 groups over 256 .. 1024 channels) .......................... group b (c: 10, 14, 16)
conv_wino_kernel
  * K loops longer than 6 steps (Ci up to 1024: 32 steps at BK 32, 64 at BK 16) ........................................... group c
  * more than 3 row blocks (8 .. 16) ...................................................................................... group c
  * Co % 32 == 16: Mp > Co, the live() == false half block, zero-sized residual and bias resources ........................ group d
  * Ci % 32 == 16: the launcher forces cfg 162, an explicit 322 is refused ................................................ group d
  * len_at(lvl) with lvl > 0, dead tiles at a level ....................................................................... group f
  * the XCD tile order on grids that are no multiple of 8, nMb and nN no powers of two .................................... group e
routing
  * the launches run_resnet routes are exactly the ones the table and its conditions name: conv1 always, conv2 only without shortcut and
    without concat, never in latency mode, a split mode or a traced run ................................................................ group g
  * "at least one" launch (test_unet_takes_the_wino_path) becomes the exact multiset of (Ci, Co, To) with one gn_wino each ............... group g
  * a table row whose launch stopped, a conv2 + shortcut that started, a latency-mode run on the planes path ............................. group g
"""
import ctypes as ct
import json
import re
from collections import Counter

import numpy as np
import pytest

import wino_numpy as W

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOL = 1e-5          # tests/test_gpu_k4p.py:198


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def relmax(a, b):
    return float(np.abs(a - b).max() / max(1e-30, np.abs(b).max()))


def U(name, shape, lo=-1.0, hi=1.0):
    from lds import init_weights
    return init_weights.uniform("wino.modes." + name, shape, 27, lo, hi)


def stream():
    return ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return None if t is None else ct.c_void_p(t.data_ptr())


def H(h):      # (host arrays)
    return None if h is None else ct.c_void_p(h.ctypes.data)


def nan_dev(n):
    return torch.full((int(n),), float("nan"), dtype=torch.float32, device="cuda")


def make_inputs(tag, B, C1, C2, Co, T):
    Ci = C1 + C2
    return dict(x1=U(f"{tag}.x1", (B, C1, T), -2, 2) + np.float32(0.3), x2=U(f"{tag}.x2", (B, C2, T), -3, 1) if C2 else None,
                gamma=U(f"{tag}.g", (Ci,), 0.5, 1.5), beta=U(f"{tag}.b", (Ci,), -0.5, 0.5), ss=U(f"{tag}.ss", (B, 2 * Ci), -0.5, 0.5),
                w=(U(f"{tag}.w", (Co, Ci, 3)) / np.float32(np.sqrt(3 * Ci))).astype(np.float32), bias=U(f"{tag}.bias", (Co,)),
                res=U(f"{tag}.res", (B, Co, T)))


def source(d):
    return d["x1"] if d["x2"] is None else np.concatenate([d["x1"], d["x2"]], axis=1)


GUARD = 4096      # floats of NaN behind the output and the partials: a store beyond the tensor lands there


class Run:
    """out [B, Co, T]; planes (device layout) or None; gp [B, Co / 16, nT, 2]; k4p: the raw K4P output [B, Co / 8, 2, T + 2, 4] (tap) or None;
    rc and the library's message; out_guard / gp_guard: the floats behind the two buffers"""


def run_wino(d, Co, groups, use_res=True, use_ss=True, lengths=None, poison=0, cfg=0, lvl=None, want_planes=True, tap=False, must_pass=True):
    from lds import native
    L = native.lib()
    B, C1, T = d["x1"].shape
    C2 = 0 if d["x2"] is None else d["x2"].shape[1]
    Ci = C1 + C2
    dx1, dx2 = dev(d["x1"]), (dev(d["x2"]) if C2 else None)
    dss, dres = (dev(d["ss"]) if use_ss else None), (dev(d["res"]) if use_res else None)
    lens = np.ascontiguousarray(lengths, dtype=np.int32) if lengths is not None else None
    Pn, nT = (T + 1) // 2, (T + 31) // 32
    n_out, n_gp = B * Co * T, B * (Co // 16) * nT * 2
    out, gp = nan_dev(n_out + GUARD), nan_dev(n_gp + GUARD)
    planes = nan_dev(B * Ci * 4 * Pn) if want_planes else None
    raw = nan_dev(B * Co * (T + 2)) if tap else None
    if tap:
        native.check(L.lds_test_tap_k4p(P(raw), raw.numel()))
    head = (P(dx1), P(dx2), C1, C2, T, H(d["gamma"]), H(d["beta"]), P(dss), groups, 1, H(d["w"]), H(d["bias"]), Co, P(dres), H(lens), poison, cfg)
    tail = (P(out), P(planes), P(gp), B, stream())
    r = Run()
    r.rc = L.lds_test_wino_conv(*head, *tail) if lvl is None else L.lds_test_wino_conv_lvl(*head, lvl, *tail)
    r.msg = L.lds_last_error().decode() if r.rc else ""
    torch.cuda.synchronize()
    if must_pass:
        native.check(r.rc)
    o, g = out.cpu().numpy(), gp.cpu().numpy()
    r.out, r.out_guard = o[:n_out].reshape(B, Co, T), o[n_out:]
    r.gp, r.gp_guard = g[:n_gp].reshape(B, Co // 16, nT, 2), g[n_gp:]
    r.planes = planes.cpu().numpy().reshape(B, Ci // 8, 2, 4, Pn, 4) if want_planes else None
    r.k4p = raw.cpu().numpy().reshape(B, Co // 8, 2, T + 2, 4) if tap else None
    return r


def gn_apply_fp32(d, groups, use_ss):
    """d = SiLU(GroupNorm(x) (* (1 + scale) + shift)) as gn_stream writes it (lds_test_gn_apply): the fp32 tensor whose transform the planes are"""
    from lds import native
    B, C1, T = d["x1"].shape
    C2 = 0 if d["x2"] is None else d["x2"].shape[1]
    out = torch.full((B, C1 + C2, T), float("nan"), dtype=torch.float32, device="cuda")
    dx1, dx2, dss = dev(d["x1"]), (dev(d["x2"]) if C2 else None), (dev(d["ss"]) if use_ss else None)
    native.check(native.lib().lds_test_gn_apply(P(dx1), P(dx2), C1, C2, T, groups, ct.c_float(1e-5), H(d["gamma"]), H(d["beta"]), P(dss), 1, P(out), B,
                                                stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def gn64(d, groups, use_ss):
    """the same tensor in float64, from the float64 statistics of every utterance's groups"""
    x, Ci = source(d), source(d).shape[1]
    return np.stack([W.gn_act(x[b], d["gamma"], d["beta"], groups, *((d["ss"][b, :Ci], d["ss"][b, Ci:]) if use_ss else (None, None)))
                     for b in range(x.shape[0])])


def conv64(dn, d, use_res):
    """float64 direct convolution of the fp32 tensor dn [B, Ci, T] (+ bias, + res)"""
    y = np.stack([W.direct(dn[b], d["w"]) for b in range(dn.shape[0])]) + d["bias"].astype(np.float64)[None, :, None]
    return y + d["res"].astype(np.float64) if use_res else y


def check_partials(out, gp, lengths=None):
    """the epilogue's (mean, M2) of every (16 channels x 32 frames) block against the output's own statistics (check_partials of
    tests/test_gpu_wino.py, its tolerances); blocks wholly beyond a length are never written.  lengths: at the tensor's level"""
    B, Co, T = out.shape
    assert gp.shape == (B, Co // 16, (T + 31) // 32, 2)
    for b in range(B):
        L = T if lengths is None else lengths[b]
        for tb in range((T + 31) // 32):
            lo, hi = tb * 32, min(L, tb * 32 + 32)
            if hi <= lo:
                assert np.isnan(gp[b, :, tb]).all(), (b, tb)
                continue
            blk = out[b, :, lo:hi].reshape(Co // 16, 16 * (hi - lo)).astype(np.float64)
            assert np.isfinite(gp[b, :, tb]).all(), (b, tb)
            assert np.abs(gp[b, :, tb, 0] - blk.mean(1)).max() < 1e-5, (b, tb)
            assert np.abs(gp[b, :, tb, 1] - ((blk - blk.mean(1, keepdims=True)) ** 2).sum(1)).max() < 1e-3, (b, tb)


def check_k4p_written(k4p, T):
    """the raw K4P output started as NaN: every entry is written, both pad frames are zero"""
    assert np.isfinite(k4p).all()
    assert not k4p[:, :, :, 0].any() and not k4p[:, :, :, T + 1].any()


def check_guards(r):
    assert np.isnan(r.out_guard).all() and np.isnan(r.gp_guard).all()


def launched_configs(fn):
    """fn() under the profiler -> (its result, the conv_wino instantiations it launched, from the records' names)"""
    from lds import native
    L = native.lib()
    native.check(L.lds_prof_enable(1))
    try:
        res = fn()
        buf = ct.create_string_buffer(1 << 16)
        native.check(L.lds_prof_summary(buf, len(buf)))
    finally:
        native.check(L.lds_prof_enable(0))
    return res, sorted(r["name"] for r in json.loads(buf.value.decode()) if r["name"].startswith("conv_wino<"))


def dense_case(tag, B, C1, C2, Co, T, groups, combos, cfg=0, tap=False):
    """one dense shape under every (use_ss, use_res) of `combos`: GroupNorm against float64, planes bit for bit, output against float64,
    partials, guards -> (the worst output error, the worst GroupNorm error)"""
    d = make_inputs(tag, B, C1, C2, Co, T)
    worst = worst_gn = 0.0
    for use_ss in sorted({c[0] for c in combos}):
        dn = gn_apply_fp32(d, groups, use_ss)
        e_gn = relmax(dn, gn64(d, groups, use_ss))
        worst_gn = max(worst_gn, e_gn)
        want_planes = W.planes_device_layout(np.stack([W.planes(dn[b]) for b in range(B)]))
        for use_res in sorted(c[1] for c in combos if c[0] == use_ss):
            r = run_wino(d, Co, groups, use_res, use_ss, cfg=cfg, tap=tap)
            assert np.isfinite(r.out).all() and np.isfinite(r.planes).all()
            # the planes are single fp32 additions of gn_stream's own values: bit for bit the restatement
            assert np.array_equal(r.planes, want_planes)
            e = relmax(r.out, conv64(dn, d, use_res))
            print(f"{tag} cfg{cfg} ss{int(use_ss)} res{int(use_res)} gn {e_gn:.3e} out {e:.3e}")
            worst = max(worst, e)
            check_partials(r.out, r.gp)
            check_guards(r)
            if tap:
                check_k4p_written(r.k4p, T)
    return worst, worst_gn


def ragged_case(tag, C1, C2, Co, T, groups, lengths, lvl, cfg=0):
    """one poisoned ragged batch at level lvl (None: lds_test_wino_conv) against every utterance alone in float64 -> (worst output error, Run, d)"""
    B = len(lengths)
    d = make_inputs(tag, B, C1, C2, Co, T)
    r = run_wino(d, Co, groups, True, True, lengths=lengths, poison=1, cfg=cfg, lvl=lvl, tap=True)
    dn, ref, L = W.ragged_reference(source(d), lengths, lvl or 0, d["gamma"], d["beta"], groups, d["w"], d["bias"], d["ss"], d["res"])
    assert np.isfinite(r.out).all() and np.isfinite(r.planes).all()
    check_k4p_written(r.k4p, T)
    worst = 0.0
    for b, n in enumerate(L):
        worst = max(worst, relmax(r.out[b, :, :n], ref[b, :, :n]))
        assert not r.out[b, :, n:].any(), (b, n)                                        # zero from the reduced length on
        want = W.planes_device_layout(W.planes(dn[b], n)[None])[0]
        assert relmax(r.planes[b], want) < TOL, (b, n)
        assert not r.planes[b][:, :, :, (n + 2) // 2:].any(), (b, n)                    # planes zero from pair (L + 2) // 2 on
    check_partials(r.out, r.gp, L)
    check_guards(r)
    print(f"{tag} lvl {lvl} lengths {lengths} -> {L} relmax {worst:.3e}")
    return worst, r, d


# ---- a. the transform pass at long T ----------------------------------------------------------------------------------------------
# 2 Pn work items per block and 256 E per pass: E = 1 up to T 256, 2 up to 512, 4 beyond; a second pass of the work loop from T 1025 on.
# cg16 ceil(T / 32) partials per group: two requests in registers (<= 128), the loop from 128 beyond.
LONG_T = [(32, 255), (32, 256), (32, 257),                   # the E 1 -> 2 boundary
          (32, 512), (32, 513),                              # the E 2 -> 4 boundary
          (32, 1024), (32, 1025), (32, 1026),                # the second pass of the work loop (odd and even T, one item and two in it)
          (16, 2048), (16, 2049),                            # 64 and 65 partials per group: the second request
          (32, 2048), (32, 2049),                            # 128 and 130 partials per group: the loop from 128
          (64, 1026)]                                        # 132 partials per group


@pytest.mark.parametrize("C,T", LONG_T)
def test_transform_pass_long_T(C, T, record_margin):
    worst, worst_gn = dense_case(f"a.{C}.{T}", 2, C, 0, 32, T, 1, [(False, True), (True, True)])
    record_margin(worst_gn, TOL, "gn")
    record_margin(worst, TOL)


def test_transform_pass_long_T_ragged(record_margin):
    """T = 2049, lengths [2049, 1030, 33]: 130 / 66 / 4 live partials per group and 2049 / 1030 / 33 valid frames -- the partial count and the
    divisor of the statistics differ per utterance"""
    worst, _, _ = ragged_case("a.ragged", 32, 0, 32, 2049, 1, [2049, 1030, 33], None)
    record_margin(worst, TOL)


# ---- b. the UNet's group layouts --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("concat", [False, True], ids=["single", "concat"])
@pytest.mark.parametrize("cpg", [32, 48, 64, 80, 96, 112, 128])
def test_group_layouts(cpg, concat, record_margin):
    """two groups of cpg channels (cg16 2 .. 8, the group of a block by the magic division by 4 .. 16); concat: the boundary of the two
    sources 16 channels inside the second group (80 per group: 96 + 64)"""
    C1, C2 = (cpg + 16, cpg - 16) if concat else (2 * cpg, 0)
    worst, worst_gn = dense_case(f"b.{cpg}.{int(concat)}", 2, C1, C2, 32, 65, 2, [(False, False), (True, True)])
    record_margin(worst_gn, TOL, "gn")
    record_margin(worst, TOL)


# ---- c. deep K, many row blocks ---------------------------------------------------------------------------------------------------
def run_direct(dn, d):
    """the direct kernel (conv_dma, lds_test_dconv) on the same fp32 tensor, weights, bias and residual"""
    from lds import native
    B, Ci, T = dn.shape
    Co = d["w"].shape[0]
    a = native.DConvTest()
    dx, dres = dev(dn), dev(d["res"])
    a.x1, a.x2, a.C1, a.C2, a.T = dx.data_ptr(), None, Ci, 0, T
    a.w, a.bias = d["w"].ctypes.data, d["bias"].ctypes.data
    a.Co, a.K, a.stride, a.pad, a.ups = Co, 3, 1, 1, 0
    a.res, a.epilogue, a.plain_out, a.v_split, a.cfg = dres.data_ptr(), 0, 0, 0, 0
    out = torch.full((B, Co, T), float("nan"), dtype=torch.float32, device="cuda")
    native.check(native.lib().lds_test_dconv(ct.byref(a), P(out), None, B, stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("cfg", [322, 162, 0])
@pytest.mark.parametrize("T", [64, 65])
@pytest.mark.parametrize("Ci,Co", [(1024, 512), (896, 384), (640, 256)])
def test_deep_k_many_row_blocks(Ci, Co, T, cfg, record_margin):
    """the UNet's widest resnet inputs, 8 groups as the UNet: 20 .. 32 K-steps at BK 32 and 40 .. 64 at BK 16, 8 .. 16 row blocks; one pair block
    (T 64) and a second with one frame in it (T 65).  The direct kernel's error on the same inputs is recorded beside Winograd's."""
    B, groups = 1, 8
    tag = f"c.{Ci}.{Co}.{T}"
    d = make_inputs(tag, B, Ci, 0, Co, T)
    dn = gn_apply_fp32(d, groups, True)
    record_margin(relmax(dn, gn64(d, groups, True)), TOL, "gn")
    ref = conv64(dn, d, True)
    r, names = launched_configs(lambda: run_wino(d, Co, groups, True, True, cfg=cfg, tap=True))
    assert len(names) == 1 and (cfg == 0 or names == [f"conv_wino<BM32 BP32 BK{cfg // 10} NST{cfg % 10}>"]), names      # the ring that was named
    assert np.isfinite(r.out).all()
    assert np.array_equal(r.planes, W.planes_device_layout(np.stack([W.planes(dn[b]) for b in range(B)])))
    check_k4p_written(r.k4p, T)
    check_partials(r.out, r.gp)
    check_guards(r)
    e_wino, e_direct = relmax(r.out, ref), relmax(run_direct(dn, d), ref)
    print(f"{tag} cfg{cfg} wino {e_wino:.3e} direct {e_direct:.3e}")
    record_margin(e_direct, TOL, "direct")
    record_margin(e_wino, TOL)


# ---- d. channel-count edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Co", [16, 48, 80])
def test_half_row_block(Co, record_margin):
    """Co % 32 == 16: the packed taps hold Mp = Co + 16 rows, the last row block's second half is not live -- its residual and bias resources
    have zero bytes, it stores nothing and writes no partial.  A partial it did write would land in the next utterance's first slot (or, from
    the last utterance, behind the buffer), a frame behind the output."""
    B, Ci, T, groups = 2, 96, 65, 2
    d = make_inputs(f"d.co{Co}", B, Ci, 0, Co, T)
    worst = 0.0
    for use_ss, use_res in ((True, True), (False, False)):
        dn = gn_apply_fp32(d, groups, use_ss)
        r = run_wino(d, Co, groups, use_res, use_ss, tap=True, want_planes=False)
        check_k4p_written(r.k4p, T)
        check_partials(r.out, r.gp)
        check_guards(r)                                     # nothing beyond Co
        worst = max(worst, relmax(r.out, conv64(dn, d, use_res)))
    record_margin(worst, TOL)


@pytest.mark.parametrize("Ci", [16, 48, 80])
def test_half_k_step(Ci, record_margin):
    """Ci % 32 == 16: the launcher's own choice (cfg 0) is BK 16 whatever the grid"""
    (worst, worst_gn), names = launched_configs(lambda: dense_case(f"d.ci{Ci}", 2, Ci, 0, 32, 65, 1, [(True, True), (False, False)], tap=True))
    assert names == ["conv_wino<BM32 BP32 BK16 NST2>"], names
    record_margin(worst_gn, TOL, "gn")
    record_margin(worst, TOL)


@pytest.mark.parametrize("Ci", [16, 48, 80])
def test_bk32_refuses_half_k_step(Ci):
    """cfg 322 by name with Ci % 32 == 16 is an error on the host: nothing of conv_wino is enqueued, the output keeps its NaN fill"""
    d = make_inputs(f"d.ci{Ci}", 2, Ci, 0, 32, 65)
    r, names = launched_configs(lambda: run_wino(d, 32, 1, True, True, cfg=322, want_planes=False, must_pass=False))
    assert r.rc != 0 and "conv_wino launch failed" in r.msg, (r.rc, r.msg)
    assert names == []
    assert np.isnan(r.out).all() and np.isnan(r.gp).all()
    check_guards(r)
    ok = run_wino(d, 32, 1, True, True, cfg=162, want_planes=False)      # the same call with the ring that fits goes through
    assert np.isfinite(ok.out).all()


# ---- e. tile order ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Co,T", [(1, 96, 130), (3, 96, 130), (5, 160, 322), (7, 96, 66)])
def test_tile_order(B, Co, T, record_margin):
    """grids of 9, 27, 150 and 42 workgroups (none a multiple of 8), nMb in {3, 5}, nN in {2, 3, 6}: every tile is computed exactly once -- a tile
    never computed leaves NaN in the output and its partials, a tile computed in another's place a mismatch"""
    nMb, nN = (Co + 31) // 32, ((T + 1) // 2 + 31) // 32
    assert (nMb * nN * B) % 8 and nMb & (nMb - 1) and (nN == 2 or nN & (nN - 1))
    worst, worst_gn = dense_case(f"e.{B}.{Co}.{T}", B, 64, 32, Co, T, 2, [(True, True)], tap=True)
    record_margin(worst_gn, TOL, "gn")
    record_margin(worst, TOL)


# ---- f. levels --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lvl,T,lengths", [(1, 65, [130, 37, 1, 129]), (2, 130, [520, 37, 259]), (3, 17, [130, 37, 1, 129])],
                         ids=["lvl1", "lvl2", "lvl3"])
def test_levels(lvl, T, lengths, record_margin):
    """level-0 lengths and lvl, as run_resnet passes them: both kernels reduce the lengths themselves.  Poisoned sources; the output is right
    inside each reduced length and zero beyond, the planes are zero from pair (L + 2) // 2 on, partials of blocks wholly beyond a length are
    untouched, the pad frames are written (ragged_case); lvl 2: utterance 1 (10 frames of 130) leaves two dead tiles.  Utterance 0 alone at
    the same level is bit-identical."""
    assert [W.level_len(n, lvl) for n in lengths][0] == T
    worst, r, d = ragged_case(f"f.{lvl}", 64, 32, 96, T, 2, lengths, lvl)
    one = {k: (v[:1] if k in ("x1", "x2", "ss", "res") and v is not None else v) for k, v in d.items()}
    alone = run_wino(one, 96, 2, True, True, lengths=lengths[:1], poison=1, lvl=lvl, tap=True)
    for got, a in ((r.out, alone.out), (r.planes, alone.planes), (r.gp, alone.gp), (r.k4p, alone.k4p)):
        assert np.array_equal(got[:1], a)
    record_margin(worst, TOL)


def test_level_entry_validates_reduced_lengths():
    """a length that leaves 1 .. T after its reduction is accepted whatever it is at level 0; one that does not is refused before any launch"""
    d = make_inputs("f.bad", 2, 32, 0, 32, 17)
    for lengths, lvl in (([130, 137], 3), ([17, 0], 0), ([130, 0], 3)):
        r = run_wino(d, 32, 1, True, True, lengths=lengths, lvl=lvl, want_planes=False, must_pass=False)
        assert r.rc != 0 and "outside 1 .. 17" in r.msg, (lengths, lvl, r.rc, r.msg)
        assert np.isnan(r.out).all()
    assert np.isfinite(run_wino(d, 32, 1, True, True, lengths=[136, 1], lvl=3, want_planes=False).out).all()


# ---- g. routing, whole UNet -------------------------------------------------------------------------------------------------------
def expected_launches(T):
    """Counter of (Ci, Co, To) over the k 3 convolutions of the resnets that run_resnet routes to conv_wino at a padded length T: the resnets of
    arch.unet_blocks at their levels' lengths ceil(T / 2^l), the table through lds_test_wino_min_T, conv1 of every resnet and conv2 only where
    the resnet has no shortcut (cin == cout) and no skip input"""
    from lds import arch, native
    down, mid, up = arch.unet_blocks(arch.unet_config())
    min_T = native.lib().lds_test_wino_min_T
    nb = len(down)
    Ts = [-(-T // 2 ** lvl) for lvl in range(nb)]
    resnets = [(cin, 0, cout, Ts[blk["idx"]]) for blk in down for cin, cout in blk["resnets"]]
    resnets += [(mid["ch"], 0, mid["ch"], Ts[nb - 1])] * 2
    resnets += [(hin, skip, cout, Ts[nb - 1 - blk["idx"]]) for blk in up for hin, skip, cout in blk["resnets"]]
    want = Counter()
    for cin, skip, cout, Tl in resnets:
        convs = [(cin + skip, cout)] + ([(cout, cout)] if cin + skip == cout and skip == 0 else [])
        for ci, co in convs:
            m = min_T(ci, co)
            if m > 0 and Tl >= m:
                want[(ci, co, Tl)] += 1
    return want


@pytest.fixture(scope="module")
def unit2mel_f32():
    from diffusion.unit2mel import Unit2Mel
    m = Unit2Mel(1280, 323, 80)
    m.to("cuda").eval()
    return m


def unet_inputs(B, T):
    from lds import init_weights
    return init_weights.uniform(f"wino.route.x{T}", (B, 336, T), 27, -2, 2), np.linspace(321.25, 17.0, B).astype(np.float32)


def profiled_forward(unet, x, t, lengths=None):
    """one forward at profiler level 2 -> (eps, Counter of (Ci, Co, To) over the conv_wino records, the count of gn_wino records)"""
    from lds import native
    L = native.lib()
    dx, dt = dev(x), dev(t)
    native.check(L.lds_prof_enable(2))
    try:
        got = unet.native().forward(dx[:, :80].contiguous(), dx[:, 80:].contiguous(), dt, lengths=lengths).cpu().numpy()
        buf = ct.create_string_buffer(1 << 20)
        native.check(L.lds_prof_summary(buf, len(buf)))
    finally:
        native.check(L.lds_prof_enable(0))
    convs, gn = Counter(), 0
    for r in json.loads(buf.value.decode()):
        if r["name"].startswith("conv_wino<"):
            m = re.search(r" Ci(\d+) Co(\d+) K3 To(\d+)", r["name"])
            assert m, r["name"]
            convs[tuple(int(v) for v in m.groups())] += r["count"]
        elif r["name"].startswith("gn_wino"):
            gn += r["count"]
    return got, convs, gn


@pytest.mark.parametrize("T", [512, 504, 129])
def test_routing_is_the_table(unit2mel_f32, T, record_margin):
    """T 512: levels 512 / 256 / 128 / 64, every row of the table at or above its minimum; T 504: 504 / 252 / 126 / 63, levels 1 to 3 just below
    theirs; T 129: the 640 -> 256 row (from 130) off while the rows from 64 are on.  The launches are exactly the predicted multiset, one
    gn_wino per conv_wino, and the output is the oracle's."""
    from lds import arch
    from oracle import unet1d as o_unet
    cfg = arch.unet_config()
    want = expected_launches(T)
    assert want, "no routed launch expected: the case checks nothing"
    unet = unit2mel_f32.decoder.denoise_fn
    x, t = unet_inputs(1, T)
    got, convs, gn = profiled_forward(unet, x, t)
    assert convs == want, (sorted((want - convs).items()), sorted((convs - want).items()))
    assert gn == sum(want.values())
    wu = {k[len("decoder.denoise_fn."):]: v.detach().cpu().numpy() for k, v in unit2mel_f32.state_dict().items() if k.startswith("decoder.denoise_fn.")}
    ref = o_unet.unet_forward(wu, cfg, arch.unet_blocks(cfg), x, t)
    assert np.isfinite(got).all()
    record_margin(relmax(got, ref), 2e-5)


def test_routing_expectation_sees_the_edges():
    """the prediction itself, from the library's table: T 512 routes rows that T 504 does not, T 129 routes no 640 -> 256, nothing with a
    shortcut or a skip input routes its conv2 (every routed square shape comes from a resnet without either)"""
    from lds import native
    w512, w504, w129 = expected_launches(512), expected_launches(504), expected_launches(129)
    assert set(k[2] for k in w512) == {512, 256, 128, 64} and set(k[2] for k in w504) < {504, 252, 126, 63}
    assert (640, 256, 512) in w512 and not [k for k in w129 if k[:2] == (640, 256)] and w129
    assert 129 < native.lib().lds_test_wino_min_T(640, 256) <= 512 and native.lib().lds_test_wino_min_T(8, 8) == 0
    assert sum(w512.values()) > sum(w504.values()) > sum(w129.values()) > 0
    # a (384, 384) resnet routes both convolutions, the (256, 384) one before it (shortcut) only its conv1; no up resnet (skip input) a conv2
    assert w512[(384, 384, 256)] == 2 and w512[(256, 384, 256)] == 1


@pytest.mark.parametrize("mode", ["latency", "split_f16", "traced"])
def test_no_routing_outside_exact_fp32(unit2mel_f32, mode):
    """latency mode, the split mode and a run under the debug trace (it decodes K4P tensors) keep the direct path at T 512, where exact-fp32
    mode routes every row: no conv_wino, no gn_wino"""
    from lds import native
    unet = unit2mel_f32.decoder.denoise_fn
    x, t = unet_inputs(1, 512)
    try:
        if mode == "latency":
            unet.set_latency_mode(True)
        elif mode == "traced":
            native.debug_trace(True)
        else:
            unet.set_gemm_mode(mode)
        got, convs, gn = profiled_forward(unet, x, t)
    finally:
        native.debug_trace(False)
        unet.set_latency_mode(False)
        unet.set_gemm_mode("f32")
    assert not convs and gn == 0, (convs, gn)
    assert np.isfinite(got).all()


def test_routing_does_not_see_lengths_or_batch(unit2mel_f32):
    """a ragged batch of four at a padded T of 512: the launches are the ones predicted for T 512 (the values are tests/test_gpu_ragged_poison.py's)"""
    lengths = [512, 300, 272, 401]
    unet = unit2mel_f32.decoder.denoise_fn
    x, t = unet_inputs(len(lengths), 512)
    got, convs, gn = profiled_forward(unet, x, t, lengths=lengths)
    want = expected_launches(512)
    assert convs == want, (sorted((want - convs).items()), sorted((convs - want).items()))
    assert gn == sum(want.values())
    assert np.isfinite(got).all()
