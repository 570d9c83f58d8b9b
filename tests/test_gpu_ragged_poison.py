"""Ragged batches under hostile padding and poisoned workspaces: the ragged UNet forward (lds_unet_forward_ragged), the ragged samplers
(lds_sampler_run_ragged, GaussianDiffusion.forward_ragged, Unit2Mel.forward_ragged) and the ragged vocoder (lds_vocoder_forward_ragged,
Hifi_VAEGAN.forward_ragged).  Each promises that every utterance equals its stand-alone run and that frames past its length are zeros,
whatever the buffers hold there.  Here the padding of every input holds NaN, +-Inf and +-1e30, and the workspace holds NaN, +Inf, fp16 /
bf16 patterns or large finite words before each call: the result must be finite, exactly zero past each length, bit-identical to the run
with finite padding over a zeroed workspace, and each utterance must match its run alone."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# the workspace fills of test_gpu_determinism.PATTERNS, plus +Inf
WS_PATTERNS = {"zeros": 0x00000000, "nan": 0x7FC07FC0, "ones": 0x3F803C00, "big": 0x7B007B00, "inf": 0x7F800000}
H_RB2 = dict(resblock="2", resblock_dilation_sizes=[[1, 3], [1, 3], [1, 3]])


def CUDA():
    """the current device with its index: the handles' workspaces are keyed by str(device)"""
    return torch.device("cuda", torch.cuda.current_device())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def relmax(got, ref):
    return float(np.abs(got.astype(np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


def _garbage(tag, n):
    """n values of the padding mix: +-1e30, NaN every 7th, +Inf and -Inf among them"""
    from lds import init_weights
    g = np.where(init_weights.uniform(tag, (n,), 91, -1.0, 1.0) < 0, np.float32(-1e30), np.float32(1e30)).astype(np.float32)
    g[::7] = np.nan
    g[3::11] = np.inf
    g[5::13] = -np.inf
    return g


def _poison(a, lens, axis, tag):
    """copy of a [B, ...] with the padding mix at index >= lens[b] along `axis` (counted without the batch axis) of every element b"""
    a = a.copy()
    for b, n in enumerate(lens):
        s = np.moveaxis(a[b], axis, -1)      # (a view: writes land in a)
        if n < s.shape[-1]:
            s[..., n:] = _garbage(f"{tag}.{b}", s[..., n:].size).reshape(s[..., n:].shape)
    return a


def _fill(ws, pattern):
    from lds import native
    native.debug_fill(ws, pattern)


def _check_padding_zero(y, lens, axis, scale=1):
    """y [B, ...] is exactly zero at index >= scale * lens[b] along `axis` (counted without the batch axis)"""
    for b, n in enumerate(lens):
        s = y[b].movedim(axis, -1)
        if scale * n < s.shape[-1]:
            assert not bool(s[..., scale * n:].any()), f"utterance {b}: nonzero values past its length {n}"


# ---- the ragged UNet forward ----------------------------------------------------------------------------------------------------
UNET_SHAPES = [(512, [512, 300, 272, 401]), (130, [64, 130, 7, 129, 2]),
               (2050, [2050, 1100])]      # (2050: a group of the first level has more than 64 partials, the fold loads further rounds)


@pytest.fixture(scope="module")
def u2m():
    from diffusion.unit2mel import Unit2Mel
    return Unit2Mel(1280, 323, 80).to("cuda").eval()


@pytest.mark.parametrize("padding", ["finite", "poison"])
@pytest.mark.parametrize("T,lens", UNET_SHAPES, ids=lambda v: str(v) if isinstance(v, int) else f"B{len(v)}")
@pytest.mark.parametrize("latency", [False, True], ids=["std", "lat"])
@pytest.mark.parametrize("mode", ["f32", "split_f16"])
def test_ragged_unet_poison(u2m, mode, latency, T, lens, padding, record_margin):
    from lds import init_weights
    unet = u2m.decoder.denoise_fn
    unet.set_gemm_mode(mode)
    unet.set_latency_mode(latency)
    try:
        B = len(lens)
        nat = unet.native()
        x = init_weights.uniform(f"rgp.{T}.{B}", (B, 336, T), 61, -2, 2)
        t = dev(np.linspace(40.5, 873.25, B).astype(np.float32))
        ws = nat.workspace_tensor(B, T, CUDA())

        def run(xa):
            dx = dev(xa)
            return nat.forward(dx[:, :80].contiguous(), dx[:, 80:].contiguous(), t, lengths=lens).clone()
        _fill(ws, 0)
        clean = run(x)
        xp = _poison(x, lens, 1, f"rgp.pad.{T}.{B}") if padding == "poison" else x
        for name, pat in WS_PATTERNS.items():
            _fill(ws, pat)
            y = run(xp)
            assert torch.isfinite(y).all(), f"workspace {name}, {padding} padding: non-finite output"
            assert torch.equal(y, clean), f"workspace {name}, {padding} padding: differs from the clean run by {relmax(y.cpu().numpy(), clean.cpu().numpy()):.2e}"
        _check_padding_zero(clean, lens, 1)
        worst = 0.0
        for b, n in enumerate(lens):
            alone = unet(dev(x[b:b + 1, :, :n]), t[b:b + 1]).sample
            worst = max(worst, relmax(clean[b:b + 1, :, :n].cpu().numpy(), alone.cpu().numpy()))
        record_margin(worst, 2e-5)
    finally:
        unet.set_latency_mode(False)
        unet.set_gemm_mode("f32")


# ---- the ragged samplers ---------------------------------------------------------------------------------------------------------
SAMPLER_CASES = [("dpm-solver", 250, 1000, 96, [96, 61, 40]), ("unipc", 250, 1000, 96, [96, 61, 40]), ("ddim", 250, 1000, 96, [96, 61, 40]),
                 ("ddpm", 1, 12, 96, [96, 61, 40]),
                 ("dpm-solver", 250, 1000, 288, [288, 150, 33])]      # (lengths 100+ frames apart: whole 32-frame blocks past a length at every level)


@pytest.mark.parametrize("method,speedup,k_step,T,lens", SAMPLER_CASES, ids=lambda v: str(v) if not isinstance(v, list) else f"B{len(v)}")
@pytest.mark.parametrize("mode", ["f32", "split_f16"])
def test_ragged_sampler_poison(u2m, monkeypatch, mode, method, speedup, k_step, T, lens, record_margin):
    """GaussianDiffusion.forward_ragged with the padding of cond, of x_T and of every DDPM noise draw poisoned and the sampler workspace
    filled with each pattern"""
    from lds import init_weights
    gd = u2m.decoder
    gd.denoise_fn.set_gemm_mode(mode)
    B = len(lens)
    meth = None if method == "ddpm" else method
    K = k_step if method == "ddpm" else 0
    cond = init_weights.uniform(f"rsp.cond.{T}", (B, T, 256), 71, -1, 1)
    xT = init_weights.uniform(f"rsp.xT.{T}", (B, 1, 80, T), 72, -1.7, 1.7)
    draws = init_weights.uniform(f"rsp.noise.{T}", (max(K, 1), B, 1, 80, T), 74, -1.7, 1.7)
    ws = gd.denoise_fn.native().workspace_tensor(B, T, CUDA(), sampler=True)
    gd.k_step = k_step

    def run(c, x0, nz):
        q = [dev(d) for d in nz[:K]]
        monkeypatch.setattr(torch, "randn", lambda *a, **k: q.pop(0))
        y = gd.forward_ragged(dev(c), lens, infer_speedup=speedup, method=meth, x_T=dev(x0)).clone()
        assert not q, "the sampler did not draw every noise tensor"
        return y
    try:
        _fill(ws, 0)
        clean = run(cond, xT, draws)
        assert clean.shape == (B, T, 80)
        cond_p = _poison(cond, lens, 0, f"rsp.pc.{T}")
        xT_p = _poison(xT, lens, 2, f"rsp.px.{T}")
        draws_p = np.stack([_poison(d, lens, 2, f"rsp.pn.{T}.{i}") for i, d in enumerate(draws)])
        for name, pat in WS_PATTERNS.items():
            _fill(ws, pat)
            y = run(cond_p, xT_p, draws_p)
            assert torch.isfinite(y).all(), f"workspace {name}: non-finite output"
            assert torch.equal(y, clean), f"workspace {name}: differs from the clean run by {relmax(y.cpu().numpy(), clean.cpu().numpy()):.2e}"
        _check_padding_zero(clean, lens, 0)
        worst = 0.0
        for b, n in enumerate(lens):
            q = [dev(d[b:b + 1, :, :, :n]) for d in draws[:K]]
            monkeypatch.setattr(torch, "randn", lambda *a, **k: q.pop(0))
            alone = gd(dev(cond[b:b + 1, :n]), infer=True, infer_speedup=speedup, method=meth, x_T=dev(xT[b:b + 1, :, :, :n]))
            worst = max(worst, relmax(clean[b:b + 1, :n].cpu().numpy(), alone.cpu().numpy()))
        record_margin(worst, 1e-4)
    finally:
        gd.k_step = 1000
        gd.denoise_fn.set_gemm_mode("f32")


def test_ragged_unit2mel_poisoned_units(u2m, record_margin):
    """Unit2Mel.forward_ragged with the units' padding poisoned: the embedding carries the poison into cond's padding, which the ragged
    sampler must never read"""
    from lds import init_weights
    T, lens = 160, [160, 97, 41]
    B = len(lens)
    units = init_weights.uniform("ru.units", (B, T, 1280), 75, -1.7, 1.7)
    xT = init_weights.uniform("ru.xT", (B, 1, 80, T), 76, -1.7, 1.7)
    spk = torch.tensor([[7], [12], [300]], dtype=torch.int64)
    kw = dict(infer_speedup=250, method="dpm-solver")
    clean = u2m.forward_ragged(dev(units), lens, spk_id=spk, x_T=dev(xT), **kw).clone()
    y = u2m.forward_ragged(dev(_poison(units, lens, 0, "ru.pu")), lens, spk_id=spk, x_T=dev(_poison(xT, lens, 2, "ru.px")), **kw)
    assert torch.isfinite(y).all()
    assert torch.equal(y, clean)
    _check_padding_zero(y, lens, 0)
    worst = 0.0
    for b, n in enumerate(lens):
        alone = u2m(dev(units[b:b + 1, :n]), None, spk_id=spk[b:b + 1], infer=True, x_T=dev(xT[b:b + 1, :, :, :n]), **kw)
        worst = max(worst, relmax(y[b:b + 1, :n].cpu().numpy(), alone.cpu().numpy()))
    record_margin(worst, 1e-4)


# ---- the ragged vocoder ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,lens", [(40, [40, 24, 33]), (96, [17, 96, 60, 1]), (512, [512, 300, 272, 401])],
                         ids=lambda v: str(v) if isinstance(v, int) else f"B{len(v)}")
@pytest.mark.parametrize("pair", [1, 0], ids=["pair", "twolaunch"])
@pytest.mark.parametrize("rb", ["1", "2"])
def test_ragged_vocoder_poison(rb, pair, T, lens, record_margin):
    """Hifi_VAEGAN.forward_ragged with z's padding poisoned and the workspace filled with each pattern, the narrow stages' residual steps
    fused (csrc/voc_pair.hip) and as two launches"""
    from encoder.hifi_vaegan.hifi_vaegan import Hifi_VAEGAN
    from lds import arch, init_weights, native
    h = arch.SYNTHETIC_VOCODER_H if rb == "1" else dict(arch.SYNTHETIC_VOCODER_H, **H_RB2)
    voc = Hifi_VAEGAN(None, device="cuda", h=h, state=init_weights.init_state(arch.generator_param_shapes(h), 0))
    B, hop = len(lens), h["hop_size"]
    z = init_weights.uniform(f"rvp.{T}", (B, T, h["inter_channels"]), 81, -1.5, 1.5)
    native.check(native.lib().lds_debug_set_voc_pair(pair))
    try:
        voc(dev(z[:1, :1]))      # (creates the native decoder)
        ws = voc.decoder_model.workspace_tensor(B, T, CUDA())
        _fill(ws, 0)
        clean = voc.forward_ragged(dev(z), lens).clone()
        assert clean.shape == (B, 1, T * hop)
        zp = dev(_poison(z, lens, 0, f"rvp.pad.{T}"))
        for name, pat in WS_PATTERNS.items():
            _fill(ws, pat)
            y = voc.forward_ragged(zp, lens)
            assert torch.isfinite(y).all(), f"workspace {name}: non-finite output"
            assert torch.equal(y, clean), f"workspace {name}: differs from the clean run by {relmax(y.cpu().numpy(), clean.cpu().numpy()):.2e}"
        _check_padding_zero(clean, lens, 1, hop)
        worst = 0.0
        for b, n in enumerate(lens):
            alone = voc(dev(z[b:b + 1, :n]))
            worst = max(worst, relmax(clean[b:b + 1, :, :n * hop].cpu().numpy(), alone.cpu().numpy()))
        record_margin(worst, 1e-4)
    finally:
        native.check(native.lib().lds_debug_set_voc_pair(1))
