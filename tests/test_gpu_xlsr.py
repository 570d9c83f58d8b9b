"""The XLSR-53 (wav2vec 2.0, layer-norm flavour) units encoder on the GPU (include/lds.h lds_w2v_*, encoder.wav2vec2.model,
tools.tools.Audio2xlsr_53_56k / Units_Encoder): the feature extractor and the encoder against the fixtures recorded from
transformers.Wav2Vec2Model in float64 (tests/golden/xlsr.npz), every frame of the long clips and a reduced configuration at 24 layers
against the numpy restatement (tests/w2v_numpy.py, pinned to the same fixtures by tests/test_cpu_xlsr.py), the two new kernels alone, the
ragged-batch invariants and the Python surface.  Weights: XLSR-53's widths with 2 layers unless stated."""
import os

import numpy as np
import pytest
import torch

import test_gpu_svc as TS
import w2v_numpy as wnp
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

TOL = 2e-5              # x absmax against the fp64 reference: the project's bound for an fp32 encoder (DESIGN sections 18, 22)
TOL_RAGGED = 1e-5       # x absmax: a clip inside a ragged batch against the clip alone, across buffer lengths
POISON = (0x7FC00000, 0x7F800000, 0xFF800000)      # NaN, +Inf, -Inf
SMALL = dict(conv_dim=64, n_state=128, n_head=2, n_layer=24, n_ffn=512, pos_kernel=128, pos_groups=8, n_ctx=1500)
RAGGED = (112077, 1279, 400)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def relmax(got, ref, absmax=None):
    return float(np.abs(got.astype(np.float64) - ref).max() / (absmax if absmax else max(np.abs(ref).max(), 1e-30)))


_Z, _STATE, _HANDLES, _CLIPS, _REF = {}, {}, {}, {}, {}


def fixtures():
    if not _Z:
        _Z.update(np.load(os.path.join(GOLDEN, "xlsr.npz")))
    return _Z


def _dims(small=False):
    from lds import arch
    return dict(SMALL) if small else dict(arch.XLSR_53_DIMS, n_layer=wnp.FIXTURE_LAYERS)


def _state(small=False):
    from lds import arch
    if small not in _STATE:
        _STATE[small] = arch.w2v_init_state(_dims(small), wnp.FIXTURE_SEED)
    return _STATE[small]


def _handle(small=False):
    from lds import native
    if small not in _HANDLES:
        _HANDLES[small] = native.Wav2Vec2(_dims(small), _state(small))
    return _HANDLES[small]


def _clip(i):
    from lds import init_weights
    if i not in _CLIPS:
        _CLIPS[i] = wnp.make_clip(i, init_weights.uniform)
    return _CLIPS[i]


def _numpy_ref(small, clip):
    """(features, encoder output) of the float64 restatement, computed once per (configuration, clip)"""
    key = (small, clip)
    if key not in _REF:
        f64 = wnp.features(_state(small), _clip(clip), np.float64)
        _REF[key] = (f64, wnp.encode(_state(small), _dims(small), _clip(clip), np.float64, feats=f64))
    return _REF[key]


def _against(name, i, got, record_margin):
    z = fixtures()
    ref, rows = z[f"{name}_{i}"].astype(np.float64), z[f"rows_{i}"]
    assert got.shape == (wnp.FRAMES[i], ref.shape[1]), (got.shape, ref.shape)
    assert np.isfinite(got).all()
    e = relmax(got[rows], ref, float(z[f"absmax_{name}_{i}"]))
    print(f"{name} clip {i}: max |native - ref64| / absmax {e:.3e} (the model's own fp32 gap {float(z[f'gap_{name}_{i}']):.2e})")
    record_margin(e, TOL, name)


@pytest.mark.parametrize("clip", [0, 1, 2, 3, 4])
def test_xlsr_features_and_encode_vs_reference(clip, record_margin):
    """lds_w2v_features and lds_w2v_encode at XLSR-53's widths with 2 layers, every recorded row of every fixture clip"""
    a = dev(_clip(clip)[None])
    _against("feat", clip, _handle().features(a)[0].cpu().numpy(), record_margin)
    _against("enc", clip, _handle().encode(a)[0].cpu().numpy(), record_margin)


@pytest.mark.parametrize("clip", [3, 4])
def test_xlsr_full_width_every_frame_vs_numpy(clip, record_margin):
    """the 192- and 349-frame clips, of which the fixtures record selected rows only: every frame against the float64 restatement (349
    frames: more than 64 frames plus the positional convolution's 127-frame window at group width 64)"""
    f64, e64 = _numpy_ref(False, clip)
    a = dev(_clip(clip)[None])
    got_f, got_e = _handle().features(a)[0].cpu().numpy(), _handle().encode(a)[0].cpu().numpy()
    assert got_f.shape == f64.shape == (wnp.FRAMES[clip], 512) and got_e.shape == e64.shape == (wnp.FRAMES[clip], 1024)
    record_margin(relmax(got_f, f64), TOL, "feat")
    record_margin(relmax(got_e, e64), TOL, "enc")


@pytest.mark.parametrize("clip", [1, 3])
def test_xlsr_reduced_configuration_24_layers_vs_numpy(clip, record_margin):
    """conv_dim 64, n_state 128, 2 heads, n_ffn 512, 8 groups of 16 channels, 24 layers: every frame against the float64 restatement"""
    f64, e64 = _numpy_ref(True, clip)
    a = dev(_clip(clip)[None])
    assert 0.1 < np.abs(e64).max() < 100 and 0.1 < np.abs(f64).max() < 100
    record_margin(relmax(_handle(True).features(a)[0].cpu().numpy(), f64), TOL, "feat")
    record_margin(relmax(_handle(True).encode(a)[0].cpu().numpy(), e64), TOL, "enc")


def _ragged_audio(fill, L=None, lens=RAGGED, order=(4, 1, 0)):
    L = max(lens) if L is None else L
    a = np.full((len(lens), L), fill, dtype=np.float32)
    for b, (n, i) in enumerate(zip(lens, order)):
        a[b, :n] = _clip(i)
    return a


def test_xlsr_ragged_vs_alone(record_margin):
    """B = 3 of 112,077 / 1,279 / 400 samples in one buffer, NaN beyond the clips: each against the clip alone (its own buffer length)
    within 1e-5 absmax, rows beyond T_b exactly zero"""
    h = _handle()
    audio = dev(_ragged_audio(np.nan))
    for what, call in (("feat", h.features), ("enc", h.encode)):
        got = call(audio, RAGGED)
        assert got.shape[:2] == (3, 349) and torch.isfinite(got).all()
        worst = 0.0
        for b, n in enumerate(RAGGED):
            T = wnp.frames_of(n)
            alone = call(audio[b:b + 1, :n].contiguous())[0]
            worst = max(worst, relmax(got[b, :T].cpu().numpy(), alone.cpu().numpy().astype(np.float64)))
            assert not got[b, T:].any(), (what, b)
        record_margin(worst + 1e-30, TOL_RAGGED, what)


def test_xlsr_same_buffer_length_is_bit_identical():
    """a clip alone in a buffer of L samples, inside B = 3 and inside B = 5 with the same L: the same bits (the tile rules are judged at
    the nominal batch); all lengths equal to L against lengths = NULL: the same bits"""
    h = _handle()
    L = max(RAGGED)
    lens5 = (400, 112077, 1279, 41277, 400)
    a3 = dev(_ragged_audio(0.0))
    a5 = dev(_ragged_audio(0.0, L, lens5, (0, 4, 1, 2, 0)))
    u3, u5 = h.encode(a3, RAGGED), h.encode(a5, lens5)
    for b, n in enumerate(RAGGED):
        one = torch.zeros(1, L, device="cuda")
        one[0, :n] = a3[b, :n]
        alone = h.encode(one, [n])[0]
        assert torch.equal(u3[b], alone), b
        assert torch.equal(u5[(1, 2, 0)[b]], alone), b
    full = dev(np.stack([_clip(2), _clip(2)[::-1].copy()]))
    assert torch.equal(h.encode(full, [41277, 41277]), h.encode(full))
    assert torch.equal(h.features(full, [41277, 41277]), h.features(full))


def test_xlsr_poison_changes_nothing():
    """NaN / 1e30 in the audio beyond lengths[b], a NaN / +Inf / -Inf workspace, five repeated calls: bit-identical to the clean run"""
    from lds import native
    h = _handle()
    clean = dev(_ragged_audio(0.0))
    ref, ref_f = h.encode(clean, RAGGED), h.features(clean, RAGGED)
    assert torch.isfinite(ref).all()
    for fill in (np.nan, 1e30):
        bad = dev(_ragged_audio(fill))
        assert torch.equal(h.encode(bad, RAGGED), ref) and torch.equal(h.features(bad, RAGGED), ref_f), fill
    bad = dev(_ragged_audio(np.nan))
    ws = torch.empty(h.workspace_bytes(3, max(RAGGED)), dtype=torch.uint8, device="cuda")
    for pat in POISON:
        native.debug_fill(ws, pat)
        assert torch.equal(h.encode(bad, RAGGED, ws=ws), ref), hex(pat)
        native.debug_fill(ws, pat)
        assert torch.equal(h.features(bad, RAGGED, ws=ws), ref_f), hex(pat)
        native.debug_fill(ws, pat)
        assert torch.equal(h.encode(bad[1:2, :1279].contiguous(), ws=ws), h.encode(clean[1:2, :1279].contiguous())), hex(pat)
    for _ in range(5):
        assert torch.equal(h.encode(bad, RAGGED), ref)


# ---- the two new kernels alone (include/lds_test.h) -------------------------------------------------------------------------------------
def _gelu64(x):
    from scipy.special import erf
    return x * 0.5 * (1.0 + erf(x / np.sqrt(2.0)))


def _ln_act64(x, g, b, eps=1e-5):
    """x [B][C][T] float64 -> GELU(LayerNorm over C)"""
    mu = x.mean(axis=1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=1, keepdims=True)
    return _gelu64((x - mu) / np.sqrt(var + eps) * g[None, :, None] + b[None, :, None])


def _host_i32(v):
    return None if v is None else np.ascontiguousarray(v, dtype=np.int32)


# frame counts 1, 79 and 254 alone, and 255 next to a ragged neighbour of 79
CASES = [(1, None), (79, None), (254, None), (255, (255, 79))]


@pytest.mark.parametrize("C_", [64, 512])
@pytest.mark.parametrize("T,lens", CASES)
def test_w2v_conv0_alone(C_, T, lens, record_margin):
    """w2v_conv0: conv0 + bias + LayerNorm over the channels + GELU against float64, zeros beyond a clip's frames whatever the audio
    holds there"""
    from lds import init_weights as iw, native
    B = 1 if lens is None else len(lens)
    L = 5 * (T - 1) + 10 + 3      # three samples that no frame reaches
    tag = f"t.w2v.conv0.{C_}.{T}"
    audio = iw.uniform(tag + ".a", (B, L), 3, -1.0, 1.0)
    w = iw.uniform(tag + ".w", (C_, 10), 3, -0.77, 0.77)
    bias, g, be = iw.uniform(tag + ".b", (C_,), 3, -0.5, 0.5), iw.uniform(tag + ".g", (C_,), 3, 0.8, 1.2), iw.uniform(tag + ".be", (C_,), 3, -0.1, 0.1)
    slen = None if lens is None else [5 * (n - 1) + 10 + 2 for n in lens]
    if slen is not None:
        for b, n in enumerate(slen):
            audio[b, n:] = np.nan
        slen[0] = L
        audio[0] = iw.uniform(tag + ".a0", (L,), 3, -1.0, 1.0)
    out = torch.empty(B, C_, T, device="cuda")
    ln = _host_i32(slen)
    d = [dev(v) for v in (audio, w, bias, g, be)]      # (kept alive over the call)
    native.check(native.lib().lds_test_w2v_conv0(native._dev(d[0]), native._host(ln), native._dev(d[1]), native._dev(d[2]), native._dev(d[3]),
                                                 native._dev(d[4]), 1e-5, native._dev(out), B, C_, L, native._stream()))
    got = out.cpu().numpy()
    a64 = np.nan_to_num(audio.astype(np.float64))
    cols = np.stack([a64[:, k:k + 5 * (T - 1) + 1:5] for k in range(10)], axis=1)      # [B][10][T]
    ref = _ln_act64(np.einsum("ck,bkt->bct", w.astype(np.float64), cols) + bias.astype(np.float64)[None, :, None], g.astype(np.float64), be.astype(np.float64))
    for b in range(B):
        n = T if lens is None else lens[b]
        assert not got[b, :, n:].any()
        ref[b, :, n:] = 0
    assert np.isfinite(got).all()
    record_margin(relmax(got, ref), TOL)


@pytest.mark.parametrize("C_", [64, 512])
@pytest.mark.parametrize("T,lens", CASES)
def test_w2v_ln_act_alone(C_, T, lens, record_margin):
    """w2v_ln_act: GELU(LayerNorm over the channels) and the (mean, M2) partials of its output over every 32 channels against float64;
    zeros (and zero partials) beyond a clip's frames whatever the input holds there"""
    from lds import init_weights as iw, native
    B = 1 if lens is None else len(lens)
    tag = f"t.w2v.ln.{C_}.{T}"
    x = iw.uniform(tag + ".x", (B, C_, T), 4, -3.0, 3.0)
    g, be = iw.uniform(tag + ".g", (C_,), 4, 0.8, 1.2), iw.uniform(tag + ".be", (C_,), 4, -0.1, 0.1)
    if lens is not None:
        for b, n in enumerate(lens):
            x[b, :, n:] = np.nan
    out = torch.empty(B, C_, T, device="cuda")
    part = torch.full((B, C_ // 32, T, 2), float("nan"), device="cuda")
    ln = _host_i32(lens)
    d = [dev(v) for v in (x, g, be)]      # (kept alive over the calls)
    for p in (part, None):
        native.check(native.lib().lds_test_w2v_ln_act(native._dev(d[0]), native._host(ln), native._dev(d[1]), native._dev(d[2]), 1e-5, native._dev(out),
                                                      native._dev_or_null(p), B, C_, T, native._stream()))
        got = out.cpu().numpy()
        ref = _ln_act64(np.nan_to_num(x.astype(np.float64)), g.astype(np.float64), be.astype(np.float64))
        for b in range(B):
            n = T if lens is None else lens[b]
            assert not got[b, :, n:].any()
            ref[b, :, n:] = 0
        assert np.isfinite(got).all()
        record_margin(relmax(got, ref), TOL, "out" if p is not None else "out.nopart")
    gp = part.cpu().numpy().astype(np.float64)
    assert np.isfinite(gp).all()
    r = ref.reshape(B, C_ // 32, 32, T)
    mean, m2 = r.mean(axis=2), ((r - r.mean(axis=2, keepdims=True)) ** 2).sum(axis=2)
    record_margin(relmax(gp[..., 0], mean), TOL, "mean")
    record_margin(relmax(gp[..., 1], m2), TOL, "m2")
    for b in range(B):
        n = T if lens is None else lens[b]
        assert not gp[b, :, n:].any()


# ---- the Python surface -----------------------------------------------------------------------------------------------------------------
def _units_encoder(small=False):
    from tools.tools import Audio2xlsr_53_56k, Units_Encoder
    return Units_Encoder("xlsr_53_56k", model=Audio2xlsr_53_56k(dims=_dims(small), state=_state(small)))


def test_xlsr_units_encoder_encode_vs_encode_ragged(record_margin):
    import cluster
    from lds import init_weights
    enc = _units_encoder()
    assert enc.min_samples == 400 and enc.model.family == "wav2vec 2.0" and enc.model.n_ctx == 1500
    wav = dev(_clip(2))
    one = enc.encode(wav, 16000)
    assert one.shape == (128, 1024) and torch.equal(one, _handle().encode(wav[None])[0])
    short = enc.encode(wav[:250].contiguous(), 16000)      # zero-padded to 400 samples as the reference does
    assert short.shape == (1, 1024) and torch.isfinite(short).all()
    batch = dev(_ragged_audio(np.nan))
    rag, n_frames = enc.encode_ragged(batch, RAGGED)
    assert n_frames.tolist() == [349, 3, 1] and rag.shape == (3, 349, 1024)
    alone = enc.encode(batch[1, :1279].contiguous(), 16000)
    record_margin(relmax(rag[1, :3].cpu().numpy(), alone.cpu().numpy().astype(np.float64)) + 1e-30, TOL_RAGGED, "short")
    assert not rag[1, 3:].any()
    long_alone = enc.encode(batch[0].contiguous(), 16000)
    record_margin(relmax(rag[0].cpu().numpy(), long_alone.cpu().numpy().astype(np.float64)) + 1e-30, TOL_RAGGED, "long")

    class Book:
        cluster_centers_ = init_weights.uniform("xlsr.tokens.book", (64, 1024), 7, -1.0, 1.0)
    tok = enc.encode_tokens(wav, 16000, Book)
    assert tok.dtype == torch.int64 and torch.equal(tok, cluster.get_cluster_result(Book, one))
    tr, nf = enc.encode_tokens_ragged(dev(_ragged_audio(0.0)), RAGGED, Book, pad_id=-1)
    assert nf.tolist() == [349, 3, 1] and (tr[2, 1:] == -1).all() and (tr[2, :1] >= 0).all()


def test_xlsr_long_audio_two_segments(record_margin):
    """infer_from_long_audio over a reduced XLSR encoder on the first two segments of the long-audio fixture's recording: it finishes, the
    result is finite, and batch_size 1 against 2 agree within the long-audio path's ragged tolerance (tests/test_gpu_svc.py: four times the
    discrepancy between the dense per-segment chain and the ragged chain, measured in the same session from entries that predate the
    method).  Where that discrepancy is zero -- at these widths no tile choice depends on the buffer length -- the bound is zero too and
    the two runs must agree bit for bit."""
    import infer_svc
    dims = dict(SMALL, n_layer=2)
    svc = infer_svc.synthetic_svc("cuda", layers=2, encoder="xlsr_53_56k", encoder_dims=dims)
    assert svc.units_encoder.encoder == "xlsr_53_56k" and svc.units_encoder.min_samples == 400
    full = TS.dev(np.load(os.path.join(GOLDEN, "svc.npz"))["clip"])
    ranges, _ = TS._segments(svc, full, 16000)
    clip = full[:(ranges[1][2] + ranges[2][1]) // 2].contiguous()
    assert len(TS._segments(svc, clip, 16000)[0]) == 2
    parent = TS.parent_chain_discrepancy(svc, clip)
    outs = []
    for bs in (1, 2):
        torch.manual_seed(1234)
        wav, rate = svc.infer_from_long_audio(clip, sr=16000, batch_size=bs, **TS.KW)
        assert rate == 44100 and wav.is_cuda and torch.isfinite(wav).all() and float(wav.abs().max()) > 0
        outs.append(wav)
    assert outs[0].shape == outs[1].shape
    diff = float((outs[0] - outs[1]).abs().max() / outs[0].abs().max())
    print(f"dense chain against ragged chain: {parent:.3e}; batch_size 1 against 2: {diff:.3e}")
    if parent > 0:
        record_margin(diff + 1e-30, 4 * parent)
    else:
        assert diff == 0.0, diff
