"""conv_wino (csrc/conv_wino.hip) and its transform pass gn_wino_kernel (csrc/k4p_ops.hip) on the GPU, through lds_test_wino_conv:
the output against a float64 direct convolution of the same fp32 inputs (bound: relmax < 1e-5, the per-kernel bound of
tests/test_gpu_k4p.py), the planes against the restatement of tests/wino_numpy.py, the epilogue's GroupNorm partials against the output's
own statistics, poisoned workspaces and padding on a ragged batch, repeatability, batch invariance, and the whole UNet with at least one
launch on the new path."""
import ctypes as ct
import json

import numpy as np
import pytest

import wino_numpy as W

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOL = 1e-5          # tests/test_gpu_k4p.py:198
GROUPS = 2          # 16 / 48 channels per group at 32 / 96 channels (GroupNorm groups hold a multiple of 16 channels)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def relmax(a, b):
    return float(np.abs(a - b).max() / max(1e-30, np.abs(b).max()))


def U(name, shape, lo=-1.0, hi=1.0):
    from lds import init_weights
    return init_weights.uniform("wino." + name, shape, 26, lo, hi)


def stream():
    return ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return None if t is None else ct.c_void_p(t.data_ptr())


def make_inputs(tag, B, C1, C2, Co, T):
    Ci = C1 + C2
    d = dict(x1=U(f"{tag}.x1", (B, C1, T), -2, 2) + np.float32(0.3), x2=U(f"{tag}.x2", (B, C2, T), -3, 1) if C2 else None,
             gamma=U(f"{tag}.g", (Ci,), 0.5, 1.5), beta=U(f"{tag}.b", (Ci,), -0.5, 0.5), ss=U(f"{tag}.ss", (B, 2 * Ci), -0.5, 0.5),
             w=(U(f"{tag}.w", (Co, Ci, 3)) / np.float32(np.sqrt(3 * Ci))).astype(np.float32), bias=U(f"{tag}.bias", (Co,)),
             res=U(f"{tag}.res", (B, Co, T)))
    return d


def run_wino(d, Co, use_res, use_ss, lengths=None, poison=0, cfg=0, want_planes=True):
    """-> (out [B,Co,T], planes (device layout) or None, gnpart [B,Co/16,nT,2])"""
    from lds import native
    B, C1, T = d["x1"].shape
    C2 = 0 if d["x2"] is None else d["x2"].shape[1]
    Ci = C1 + C2
    dx1, dx2 = dev(d["x1"]), (dev(d["x2"]) if C2 else None)
    dss, dres = (dev(d["ss"]) if use_ss else None), (dev(d["res"]) if use_res else None)
    lens = np.ascontiguousarray(lengths, dtype=np.int32) if lengths is not None else None
    Pn, nT = (T + 1) // 2, (T + 31) // 32
    out = torch.full((B, Co, T), float("nan"), dtype=torch.float32, device="cuda")
    planes = torch.full((B, Ci // 8, 2, 4, Pn, 4), float("nan"), dtype=torch.float32, device="cuda") if want_planes else None
    gp = torch.full((B, Co // 16, nT, 2), float("nan"), dtype=torch.float32, device="cuda")
    H = lambda h: None if h is None else ct.c_void_p(h.ctypes.data)      # noqa: E731  (host arrays)
    native.check(native.lib().lds_test_wino_conv(P(dx1), P(dx2), C1, C2, T, H(d["gamma"]), H(d["beta"]), P(dss), GROUPS, 1, H(d["w"]), H(d["bias"]), Co,
                                                 P(dres), H(lens), poison, cfg, P(out), P(planes), P(gp), B, stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy(), (planes.cpu().numpy() if want_planes else None), gp.cpu().numpy()


def gn_reference_fp32(d, use_ss):
    """d = SiLU(GroupNorm(x) (* (1 + scale) + shift)) as gn_stream writes it (lds_test_gn_apply): the fp32 tensor whose transform the planes are"""
    from lds import native
    B, C1, T = d["x1"].shape
    C2 = 0 if d["x2"] is None else d["x2"].shape[1]
    out = torch.full((B, C1 + C2, T), float("nan"), dtype=torch.float32, device="cuda")
    dx1, dx2, dss = dev(d["x1"]), (dev(d["x2"]) if C2 else None), (dev(d["ss"]) if use_ss else None)
    native.check(native.lib().lds_test_gn_apply(P(dx1), P(dx2), C1, C2, T, GROUPS, ct.c_float(1e-5), ct.c_void_p(d["gamma"].ctypes.data),
                                                ct.c_void_p(d["beta"].ctypes.data), P(dss), 1, P(out), B, stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check_partials(out, gp, lengths=None):
    """the epilogue's (mean, M2) of every (16 channels x 32 frames) block against the output's own statistics (tolerances of
    tests/test_gpu_k4p.py:168-169); blocks wholly beyond a length are never written"""
    B, Co, T = out.shape
    for b in range(B):
        L = T if lengths is None else lengths[b]
        for tb in range((T + 31) // 32):
            lo, hi = tb * 32, min(L, tb * 32 + 32)
            if hi <= lo:
                assert np.isnan(gp[b, :, tb]).all()
                continue
            blk = out[b, :, lo:hi].reshape(Co // 16, 16 * (hi - lo)).astype(np.float64)
            assert np.isfinite(gp[b, :, tb]).all()
            assert np.abs(gp[b, :, tb, 0] - blk.mean(1)).max() < 1e-5
            assert np.abs(gp[b, :, tb, 1] - ((blk - blk.mean(1, keepdims=True)) ** 2).sum(1)).max() < 1e-3


SOURCES = {"c32": (32, 0), "c96": (96, 0), "c64+32": (64, 32)}


@pytest.mark.parametrize("T", [1, 2, 3, 63, 64, 65, 130])
@pytest.mark.parametrize("Co", [32, 96])
@pytest.mark.parametrize("src", list(SOURCES))
def test_wino_conv(src, Co, T, record_margin):
    B = 2
    C1, C2 = SOURCES[src]
    d = make_inputs(f"{src}.{Co}.{T}", B, C1, C2, Co, T)
    worst = 0.0
    for use_ss in (False, True):
        dn = gn_reference_fp32(d, use_ss)                                  # fp32 [B, Ci, T]
        want_planes = W.planes_device_layout(np.stack([W.planes(dn[b]) for b in range(B)]))
        conv64 = np.stack([W.direct(dn[b], d["w"]) for b in range(B)]) + d["bias"].astype(np.float64)[None, :, None]
        for use_res in (False, True):
            out, planes, gp = run_wino(d, Co, use_res, use_ss)
            ref = conv64 + (d["res"].astype(np.float64) if use_res else 0.0)
            assert np.isfinite(out).all() and np.isfinite(planes).all()
            # the planes are single fp32 additions of gn_stream's own values: bit for bit the restatement
            assert np.array_equal(planes, want_planes)
            e = relmax(out, ref)
            print(f"{src} Co{Co} T{T} ss{int(use_ss)} res{int(use_res)} relmax {e:.3e}")
            worst = max(worst, e)
            check_partials(out, gp)
    record_margin(worst, TOL)


@pytest.mark.parametrize("cfg", [162, 322])
def test_wino_conv_both_rings(cfg, record_margin):
    """each instantiation by name (the launcher picks by the grid at the nominal batch): odd length, concat, more K-steps than stages"""
    B, C1, C2, Co, T = 2, 64, 32, 96, 65
    d = make_inputs(f"ring{cfg}", B, C1, C2, Co, T)
    dn = gn_reference_fp32(d, True)
    ref = np.stack([W.direct(dn[b], d["w"]) for b in range(B)]) + d["bias"].astype(np.float64)[None, :, None] + d["res"]
    out, _, gp = run_wino(d, Co, True, True, cfg=cfg, want_planes=False)
    assert np.isfinite(out).all()
    check_partials(out, gp)
    record_margin(relmax(out, ref), TOL)


def silu64(x):
    return x / (1.0 + np.exp(-x))


def test_wino_ragged_poisoned(record_margin):
    """lengths more than 32 frames apart (130 and 37 of 130): the sources' pad frames and their frames beyond the lengths hold NaN / Inf, the
    planes, the output buffer and the partial buffers start as NaN -- every output frame and every partial inside a length is finite and right,
    everything beyond a length is zero, the K4P pad frames of the output are written"""
    from lds import native
    B, C1, C2, Co, T = 2, 64, 32, 96, 130
    lengths = [130, 37]
    d = make_inputs("ragged", B, C1, C2, Co, T)
    x = np.concatenate([d["x1"], d["x2"]], axis=1).astype(np.float64)
    Ci = C1 + C2
    raw = torch.full((B * Co * (T + 2),), float("nan"), dtype=torch.float32, device="cuda")
    native.check(native.lib().lds_test_tap_k4p(P(raw), raw.numel()))
    out, planes, gp = run_wino(d, Co, True, True, lengths=lengths, poison=1)
    assert np.isfinite(out).all() and np.isfinite(planes).all()
    k4p = raw.cpu().numpy().reshape(B, Co // 8, 2, T + 2, 4)
    assert np.isfinite(k4p).all()
    assert not k4p[:, :, :, 0].any() and not k4p[:, :, :, T + 1].any()
    worst = 0.0
    for b, L in enumerate(lengths):
        # the utterance alone, in float64: GroupNorm over its own frames, scale / shift, SiLU, direct convolution, bias, residual
        xb = x[b, :, :L].reshape(GROUPS, -1)
        xn = ((xb - xb.mean(1, keepdims=True)) / np.sqrt(xb.var(1, keepdims=True) + 1e-5)).reshape(Ci, L)
        xn = xn * d["gamma"].astype(np.float64)[:, None] + d["beta"].astype(np.float64)[:, None]
        xn = xn * (1.0 + d["ss"][b, :Ci].astype(np.float64)[:, None]) + d["ss"][b, Ci:].astype(np.float64)[:, None]
        dn = silu64(xn)
        ref = W.direct(dn, d["w"]) + d["bias"].astype(np.float64)[:, None] + d["res"][b, :, :L]
        worst = max(worst, relmax(out[b, :, :L], ref))
        assert not out[b, :, L:].any()
        want = W.planes_device_layout(W.planes(np.pad(dn, ((0, 0), (0, T - L))), L)[None])[0]
        assert relmax(planes[b], want) < TOL
        assert not planes[b][:, :, :, (L + 2) // 2:].any()
    print(f"ragged poisoned relmax {worst:.3e}")
    check_partials(out, gp, lengths)
    record_margin(worst, TOL)


@pytest.mark.parametrize("T", [512, 576])      # 256 and 288 workgroups of conv_wino (2 row blocks x T / 64 frame blocks x 16)
def test_wino_repeats_are_bit_identical(T, record_margin):
    """... and the first run is right: the E = 2 (T 512) and E = 4 (T 576) instantiations of the transform pass against float64"""
    B, C, Co = 16, 64, 64
    d = make_inputs(f"rep{T}", B, C, 0, Co, T)
    first = run_wino(d, Co, True, True, want_planes=False)
    assert np.isfinite(first[0]).all()
    dn = gn_reference_fp32(d, True)
    ref = np.stack([W.direct(dn[b], d["w"]) for b in range(B)]) + d["bias"].astype(np.float64)[None, :, None] + d["res"]
    check_partials(first[0], first[2])
    record_margin(relmax(first[0], ref), TOL)
    for _ in range(7):
        again = run_wino(d, Co, True, True, want_planes=False)
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[2], again[2])


def test_wino_batch_invariance():
    """utterance 0 alone against the same utterance inside B = 3: bit-identical"""
    B, C1, C2, Co, T = 3, 64, 32, 96, 130
    d = make_inputs("binv", B, C1, C2, Co, T)
    full = run_wino(d, Co, True, True)
    one = {k: (v[:1] if k in ("x1", "x2", "ss", "res") and v is not None else v) for k, v in d.items()}
    alone = run_wino(one, Co, True, True)
    for f, a in zip(full, alone):
        assert np.array_equal(f[:1], a)


@pytest.fixture(scope="module")
def unit2mel_f32():
    from diffusion.unit2mel import Unit2Mel
    m = Unit2Mel(1280, 323, 80)
    m.to("cuda").eval()
    return m


@pytest.mark.parametrize("B,T", [(2, 64), (1, 130)])
def test_unet_takes_the_wino_path(unit2mel_f32, B, T, record_margin):
    """the whole UNet in exact-fp32 mode against the oracle at 2e-5, and -- by the profiler's kernel names -- at least one launch on conv_wino:
    the test does not pass by falling back"""
    from lds import arch, init_weights, native
    from oracle import unet1d as o_unet
    cfg = arch.unet_config()
    blocks = arch.unet_blocks(cfg)
    w = {k: v.detach().cpu().numpy() for k, v in unit2mel_f32.state_dict().items()}
    wu = {k[len("decoder.denoise_fn."):]: v for k, v in w.items() if k.startswith("decoder.denoise_fn.")}
    x = init_weights.uniform(f"wino.unet.x{T}", (B, 336, T), 26, -2, 2)
    t = np.array([321.25, 17.0][:B], dtype=np.float32)
    unet = unit2mel_f32.decoder.denoise_fn
    L = native.lib()
    native.check(L.lds_prof_enable(1))
    try:
        got = unet(dev(x), dev(t)).sample.cpu().numpy()
        buf = ct.create_string_buffer(1 << 18)
        native.check(L.lds_prof_summary(buf, len(buf)))
    finally:
        native.check(L.lds_prof_enable(0))
    names = {r["name"]: r["count"] for r in json.loads(buf.value.decode())}
    assert any(n.startswith("conv_wino<") for n in names), sorted(names)
    assert any(n == "gn_wino" for n in names), sorted(names)
    ref = o_unet.unet_forward(wu, cfg, blocks, x, t)
    assert np.isfinite(got).all()
    record_margin(relmax(got, ref), 2e-5)
