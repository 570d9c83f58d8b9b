"""A resnet's conv2 + 1x1 shortcut as one conv_wino launch over Cm + Cin / 2 channels (csrc/model.hip run_wconv_pair; the two GroupNorm passes
csrc/k4p_ops.hip gn_wino_pair_kernel) on the GPU, through lds_test_wino_pair, and its routing in the whole UNet.

Bounds (tests/test_gpu_wino.py): output relmax < 1e-5 against a float64 direct computation of the same fp32 inputs, every utterance alone;
epilogue partials 1e-5 (mean) / 1e-3 (M2).  conv1's planes are bit-equal to lds_test_wino_conv's (the pass without the side output); the
shortcut's planes are np.array_equal to numpy's single fp32 operations (tests/wino_pair_numpy.py); conv2's planes are the transform of
lds_test_gn_apply's output (dense, bit-equal).  Output, plane and partial buffers start as NaN with a NaN guard behind each."""
import ctypes as ct
import json
import re
from collections import Counter

import numpy as np
import pytest

import wino_numpy as W
import wino_pair_numpy as WP

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOL = 1e-5          # tests/test_gpu_wino.py
GROUPS = 2
GUARD = 4096        # floats of NaN behind every buffer the kernels write


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def relmax(a, b):
    return float(np.abs(a - b).max() / max(1e-30, np.abs(b).max()))


def U(name, shape, lo=-1.0, hi=1.0):
    from lds import init_weights
    return init_weights.uniform("wino.pair." + name, shape, 30, lo, hi)


def stream():
    return ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return None if t is None else ct.c_void_p(t.data_ptr())


def H(h):
    return None if h is None else ct.c_void_p(h.ctypes.data)


def nan_dev(n):
    return torch.full((int(n),), float("nan"), dtype=torch.float32, device="cuda")


def make_inputs(tag, B, Cm, C1, C2, T):
    Cin = C1 + C2
    return dict(h=U(f"{tag}.h", (B, Cm, T), -2, 2) + np.float32(0.2), x1=U(f"{tag}.x1", (B, C1, T), -2, 2) + np.float32(0.3),
                x2=U(f"{tag}.x2", (B, C2, T), -3, 1) if C2 else None,
                gamma1=U(f"{tag}.g1", (Cin,), 0.5, 1.5), beta1=U(f"{tag}.b1", (Cin,), -0.5, 0.5),
                gamma2=U(f"{tag}.g2", (Cm,), 0.5, 1.5), beta2=U(f"{tag}.b2", (Cm,), -0.5, 0.5), ss=U(f"{tag}.ss", (B, 2 * Cm), -0.5, 0.5),
                w2=(U(f"{tag}.w2", (Cm, Cm, 3)) / np.float32(np.sqrt(3 * Cm))).astype(np.float32), b2=U(f"{tag}.bias2", (Cm,)),
                ws=(U(f"{tag}.ws", (Cm, Cin)) / np.float32(np.sqrt(Cin))).astype(np.float32), bs=U(f"{tag}.biass", (Cm,)))


def source(d):
    return d["x1"] if d["x2"] is None else np.concatenate([d["x1"], d["x2"]], axis=1)


class Run:
    """out [B, Cm, T]; v1: conv1's planes; pp: the launch's planes [B, (Cm + Cin/2)/8, 2, 4, P, 4]; gp [B, Cm/16, nT, 2]; k4p: the raw output"""


def run_pair(d, lengths=None, poison=0, cfg=0, lvl=0, tap=False):
    from lds import native
    L = native.lib()
    B, Cm, T = d["h"].shape
    C1 = d["x1"].shape[1]
    C2 = 0 if d["x2"] is None else d["x2"].shape[1]
    Cin, Ck = C1 + C2, Cm + (C1 + C2) // 2
    Pn, nT = (T + 1) // 2, (T + 31) // 32
    n_out, n_gp, n_v1, n_pp = B * Cm * T, B * (Cm // 16) * nT * 2, B * Cin * 4 * Pn, B * Ck * 4 * Pn
    out, gp, v1, pp = nan_dev(n_out + GUARD), nan_dev(n_gp + GUARD), nan_dev(n_v1 + GUARD), nan_dev(n_pp + GUARD)
    raw = nan_dev(B * Cm * (T + 2)) if tap else None
    if tap:
        native.check(L.lds_test_tap_k4p(P(raw), raw.numel()))
    lens = np.ascontiguousarray(lengths, dtype=np.int32) if lengths is not None else None
    dh, dx1, dx2, dss = dev(d["h"]), dev(d["x1"]), (dev(d["x2"]) if C2 else None), dev(d["ss"])
    native.check(L.lds_test_wino_pair(P(dh), P(dx1), P(dx2), Cm, C1, C2, T, H(d["gamma1"]), H(d["beta1"]), H(d["gamma2"]), H(d["beta2"]), P(dss), GROUPS,
                                      H(d["w2"]), H(d["b2"]), H(d["ws"]), H(d["bs"]), H(lens), poison, cfg, lvl, P(out), P(v1), P(pp), P(gp), B, stream()))
    torch.cuda.synchronize()
    r = Run()
    for name, t, n, shape in (("out", out, n_out, (B, Cm, T)), ("gp", gp, n_gp, (B, Cm // 16, nT, 2)), ("v1", v1, n_v1, (B, Cin // 8, 2, 4, Pn, 4)),
                              ("pp", pp, n_pp, (B, Ck // 8, 2, 4, Pn, 4))):
        a = t.cpu().numpy()
        assert np.isnan(a[n:]).all(), f"a store behind {name}"
        setattr(r, name, a[:n].reshape(shape))
    r.k4p = raw.cpu().numpy().reshape(B, Cm // 8, 2, T + 2, 4) if tap else None
    return r


def gn_apply_fp32(x, gamma, beta, ss):
    """SiLU(GroupNorm(x) (* (1 + scale) + shift)) as gn_stream writes it (lds_test_gn_apply)"""
    from lds import native
    B, C, T = x.shape
    out = torch.full((B, C, T), float("nan"), dtype=torch.float32, device="cuda")
    dx, dss = dev(x), (dev(ss) if ss is not None else None)
    native.check(native.lib().lds_test_gn_apply(P(dx), None, C, 0, T, GROUPS, ct.c_float(1e-5), H(gamma), H(beta), P(dss), 1, P(out), B, stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def conv1_planes_without_side(d):
    """conv1's planes from lds_test_wino_conv: gn_wino_kernel as it was, no side output"""
    from lds import native
    B, C1, T = d["x1"].shape
    C2 = 0 if d["x2"] is None else d["x2"].shape[1]
    Cin, Pn = C1 + C2, (T + 1) // 2
    out, planes = nan_dev(B * 32 * T), nan_dev(B * Cin * 4 * Pn)
    w = np.zeros((32, Cin, 3), dtype=np.float32)
    dx1, dx2 = dev(d["x1"]), (dev(d["x2"]) if C2 else None)
    native.check(native.lib().lds_test_wino_conv(P(dx1), P(dx2), C1, C2, T, H(d["gamma1"]), H(d["beta1"]), None, GROUPS, 1, H(w), None, 32, None, None, 0, 0,
                                                 P(out), P(planes), None, B, stream()))
    torch.cuda.synchronize()
    return planes.cpu().numpy().reshape(B, Cin // 8, 2, 4, Pn, 4)


def reference(d, lengths=None, lvl=0):
    """every utterance alone and cut to its reduced length, float64 -> (Y [B, Cm, T], L [B])"""
    B, Cm, T = d["h"].shape
    x = source(d)
    L = [T if lengths is None else W.level_len(lengths[b], lvl) for b in range(B)]
    Y = np.zeros((B, Cm, T))
    for b, n in enumerate(L):
        a = W.gn_act(d["h"][b, :, :n], d["gamma2"], d["beta2"], GROUPS, d["ss"][b, :Cm], d["ss"][b, Cm:])
        Y[b, :, :n] = WP.pair_direct(a, x[b, :, :n], d["w2"], d["ws"]) + (d["b2"].astype(np.float64) + d["bs"].astype(np.float64))[:, None]
    return Y, L


def check_partials(out, gp, L):
    B, Co, T = out.shape
    for b in range(B):
        for tb in range((T + 31) // 32):
            lo, hi = tb * 32, min(L[b], tb * 32 + 32)
            if hi <= lo:
                assert np.isnan(gp[b, :, tb]).all()
                continue
            blk = out[b, :, lo:hi].reshape(Co // 16, 16 * (hi - lo)).astype(np.float64)
            assert np.isfinite(gp[b, :, tb]).all()
            assert np.abs(gp[b, :, tb, 0] - blk.mean(1)).max() < 1e-5
            assert np.abs(gp[b, :, tb, 1] - ((blk - blk.mean(1, keepdims=True)) ** 2).sum(1)).max() < 1e-3


def side_layout(x, L):
    """x [B, Cin, T] fp32 -> the shortcut's blocks of the launch's planes [B, Cin/16, 2, 4, P, 4]"""
    return W.planes_device_layout(np.stack([WP.side_planes(x[b], L[b]) for b in range(x.shape[0])]))


# (C1, C2): the concat boundary inside half A, inside half B, on the half boundary; one source
SOURCES = {"c32": (32, 0), "c16+48": (16, 48), "c48+16": (48, 16), "c32+32": (32, 32)}


@pytest.mark.parametrize("T", [7, 64, 65, 130])
@pytest.mark.parametrize("Cm", [32, 96])
@pytest.mark.parametrize("src", list(SOURCES))
def test_pair_dense(src, Cm, T, record_margin):
    B = 2
    C1, C2 = SOURCES[src]
    d = make_inputs(f"{src}.{Cm}.{T}", B, Cm, C1, C2, T)
    r = run_pair(d)
    ref, L = reference(d)
    assert np.isfinite(r.out).all() and np.isfinite(r.v1).all() and np.isfinite(r.pp).all()
    # conv1's planes: bit for bit the pass without the side output
    assert np.array_equal(r.v1, conv1_planes_without_side(d))
    # the shortcut's planes: numpy's single fp32 operations on the raw input
    assert np.array_equal(r.pp[:, Cm // 8:], side_layout(source(d), L))
    # conv2's planes: the transform of gn_stream's own fp32 values
    dn = gn_apply_fp32(d["h"], d["gamma2"], d["beta2"], d["ss"])
    assert np.array_equal(r.pp[:, :Cm // 8], W.planes_device_layout(np.stack([W.planes(dn[b]) for b in range(B)])))
    e = relmax(r.out, ref)
    print(f"{src} Cm{Cm} T{T} relmax {e:.3e}")
    check_partials(r.out, r.gp, L)
    record_margin(e, TOL)


@pytest.mark.parametrize("cfg", [162, 322])
def test_pair_both_rings(cfg, record_margin):
    """each instantiation by name: Cm + Cin / 2 = 96 + 32 = 128, four (BK 32) and eight (BK 16) K-steps, odd length, concat"""
    d = make_inputs(f"ring{cfg}", 2, 96, 16, 48, 65)
    r = run_pair(d, cfg=cfg)
    ref, L = reference(d)
    check_partials(r.out, r.gp, L)
    record_margin(relmax(r.out, ref), TOL)


def test_pair_depth_48_picks_bk16(record_margin):
    """Cm + Cin / 2 = 48 is no multiple of 32: the launcher's own choice must be the BK 16 ring, and an explicit 322 is refused"""
    from lds import native
    d = make_inputs("bk16", 2, 32, 32, 0, 65)
    L = native.lib()
    L.lds_prof_enable(1)
    try:
        r = run_pair(d)
        buf = ct.create_string_buffer(1 << 16)
        native.check(L.lds_prof_summary(buf, len(buf)))
    finally:
        L.lds_prof_enable(0)
    names = [x["name"] for x in json.loads(buf.value.decode())]
    assert [n for n in names if n.startswith("conv_wino_pair<")] == ["conv_wino_pair<BM32 BP32 BK16 NST2>"], names
    assert "gn_wpair" in names and "gn_wino" in names
    record_margin(relmax(r.out, reference(d)[0]), TOL)
    with pytest.raises(Exception):
        run_pair(d, cfg=322)


@pytest.mark.parametrize("lvl,T,lengths", [(0, 130, [130, 99, 1]), (1, 65, [130, 68, 1])])
def test_pair_ragged_poisoned(lvl, T, lengths, record_margin):
    """lengths [T, T - 31, 1] at the level (level-0 lengths for lvl 1): NaN / Inf in the sources' pad frames and beyond the lengths, every
    buffer NaN before the run.  Inside a length everything is finite and right, beyond it zero; the pad frames of the output are written;
    utterance 0 alone is bit-identical."""
    B, Cm, C1, C2 = 3, 96, 48, 16
    d = make_inputs(f"rag{lvl}", B, Cm, C1, C2, T)
    r = run_pair(d, lengths=lengths, poison=1, lvl=lvl, tap=True)
    ref, L = reference(d, lengths, lvl)
    assert L == [T, T - 31, 1]
    assert np.isfinite(r.out).all() and np.isfinite(r.pp).all() and np.isfinite(r.v1).all() and np.isfinite(r.k4p).all()
    assert not r.k4p[:, :, :, 0].any() and not r.k4p[:, :, :, T + 1].any()
    assert np.array_equal(r.pp[:, Cm // 8:], side_layout(source(d), L))
    worst = 0.0
    for b, n in enumerate(L):
        worst = max(worst, relmax(r.out[b, :, :n], ref[b, :, :n]))
        assert not r.out[b, :, n:].any()
        assert not r.pp[b, :, :, :, (n + 2) // 2:].any()
    check_partials(r.out, r.gp, L)
    one = {k: (v[:1] if k in ("h", "x1", "x2", "ss") and v is not None else v) for k, v in d.items()}
    alone = run_pair(one, lengths=lengths[:1], poison=1, lvl=lvl, tap=True)
    for got, a in ((r.out, alone.out), (r.pp, alone.pp), (r.v1, alone.v1), (r.gp, alone.gp), (r.k4p, alone.k4p)):
        assert np.array_equal(got[:1], a)
    record_margin(worst, TOL)


# ---- routing, whole UNet ----------------------------------------------------------------------------------------------------------
def expected_pairs(T):
    """Counter of (Cin, Cm, To) over the resnets with a shortcut whose conv2 + shortcut run_resnet routes to conv_wino_pair at a padded length
    T: conv1 routed (lds_test_wino_min_T) and the pair's own table (lds_test_wino_pair_min_T)"""
    from lds import arch, native
    down, mid, up = arch.unet_blocks(arch.unet_config())
    L = native.lib()
    nb = len(down)
    Ts = [-(-T // 2 ** lvl) for lvl in range(nb)]
    resnets = [(cin, cout, Ts[blk["idx"]]) for blk in down for cin, cout in blk["resnets"]]
    resnets += [(hin + skip, cout, Ts[nb - 1 - blk["idx"]]) for blk in up for hin, skip, cout in blk["resnets"]]
    want = Counter()
    for cin, cout, Tl in resnets:
        m1, mp = L.lds_test_wino_min_T(cin, cout), L.lds_test_wino_pair_min_T(cin, cout)
        if cin != cout and m1 > 0 and mp > 0 and Tl >= max(m1, mp):
            want[(cin, cout, Tl)] += 1
    return want


@pytest.fixture(scope="module")
def unit2mel_f32():
    from diffusion.unit2mel import Unit2Mel
    m = Unit2Mel(1280, 323, 80)
    m.to("cuda").eval()
    return m


def unet_inputs(B, T):
    from lds import init_weights
    return init_weights.uniform(f"wino.pair.route.x{T}", (B, 336, T), 30, -2, 2), np.linspace(321.25, 17.0, B).astype(np.float32)


def profiled_forward(unet, x, t, lengths=None):
    """one forward at profiler level 2 -> (eps, Counter of (Cin, Cm, To) over the conv_wino_pair records, the count of gn_wpair records)"""
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
    pairs, gn = Counter(), 0
    for r in json.loads(buf.value.decode()):
        if r["name"].startswith("conv_wino_pair<"):
            m = re.search(r" Ci(\d+) Co(\d+) K3 To(\d+)", r["name"])
            assert m, r["name"]
            pairs[tuple(int(v) for v in m.groups())] += r["count"]
        elif r["name"].startswith("gn_wpair"):
            gn += r["count"]
    return got, pairs, gn


@pytest.mark.parametrize("T", [512, 129])
def test_unet_pair_routing_is_the_table(unit2mel_f32, T, record_margin):
    """the conv_wino_pair launches are exactly the predicted multiset, one gn_wpair each, and the output is the oracle's within 2e-5"""
    from lds import arch
    from oracle import unet1d as o_unet
    cfg = arch.unet_config()
    want = expected_pairs(T)
    if T == 512:
        assert want, "no routed pair expected at T 512: the case checks nothing"
    unet = unit2mel_f32.decoder.denoise_fn
    x, t = unet_inputs(1, T)
    got, pairs, gn = profiled_forward(unet, x, t)
    assert pairs == want, (sorted((want - pairs).items()), sorted((pairs - want).items()))
    assert gn == sum(want.values())
    wu = {k[len("decoder.denoise_fn."):]: v.detach().cpu().numpy() for k, v in unit2mel_f32.state_dict().items() if k.startswith("decoder.denoise_fn.")}
    ref = o_unet.unet_forward(wu, cfg, arch.unet_blocks(cfg), x, t)
    assert np.isfinite(got).all()
    record_margin(relmax(got, ref), 2e-5)


@pytest.mark.parametrize("mode", ["latency", "split_f16", "traced"])
def test_no_pair_routing_outside_exact_fp32(unit2mel_f32, mode):
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
        got, pairs, gn = profiled_forward(unet, x, t)
    finally:
        native.debug_trace(False)
        unet.set_latency_mode(False)
        unet.set_gemm_mode("f32")
    assert not pairs and gn == 0, (pairs, gn)
    assert np.isfinite(got).all()


def test_pair_routing_does_not_see_lengths_or_batch(unit2mel_f32):
    lengths = [512, 300, 272, 401]
    unet = unit2mel_f32.decoder.denoise_fn
    x, t = unet_inputs(len(lengths), 512)
    got, pairs, gn = profiled_forward(unet, x, t, lengths=lengths)
    want = expected_pairs(512)
    assert pairs == want, (sorted((want - pairs).items()), sorted((pairs - want).items()))
    assert gn == sum(want.values())
    assert np.isfinite(got).all()
