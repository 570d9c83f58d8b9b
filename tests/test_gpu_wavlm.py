"""The WavLM units encoder on the GPU (include/lds.h lds_wavlm_*, encoder.wavlm.model, tools.tools.WavLMUnits / Units_Encoder): both flavours
against the fixtures recorded from transformers.WavLMModel in float64 (tests/golden/wavlm.npz), the gated-bias attention alone against
numpy in float64 and, with a zero table, against the plain attention kernel bit for bit, the ragged-batch invariants, the limits and the
Python surface.  Weights: WavLM-Base+'s / WavLM-Large's widths with 2 layers."""
import os
import signal

import numpy as np
import pytest
import torch

import wavlm_numpy as wnp
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

TOL = 2e-5              # x absmax against the fp64 reference: the project's bound for an fp32 encoder (tests/test_gpu_hubert.py)
TOL_RAGGED = 1e-5       # x absmax: a clip inside a ragged batch against the clip alone, across buffer lengths
POISON = (0x7FC00000, 0x7F800000, 0xFF800000)      # NaN, +Inf, -Inf
RAGGED = (112240, 1040, 400)      # 350, 3 and 1 frames: fixture clip 4, its first 1,040 samples, fixture clip 0
LIMIT_S = 120           # every test's own time limit


@pytest.fixture(autouse=True)
def time_limit():
    def on_alarm(signum, frame):
        raise TimeoutError(f"test exceeded its time limit of {LIMIT_S} s")
    old = signal.signal(signal.SIGALRM, on_alarm)
    signal.alarm(LIMIT_S)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def relmax(got, ref, absmax=None):
    return float(np.abs(got.astype(np.float64) - ref).max() / (absmax if absmax else max(np.abs(ref).max(), 1e-30)))


_Z, _STATE, _HANDLES, _CLIPS = {}, {}, {}, {}


def fixtures():
    if not _Z:
        _Z.update(np.load(os.path.join(GOLDEN, "wavlm.npz")))
    return _Z


def _dims(flavour):
    from lds import arch
    return wnp.dims_of(flavour, arch)


def _state(flavour):
    from lds import arch
    if flavour not in _STATE:
        _STATE[flavour] = arch.wavlm_init_state(_dims(flavour), wnp.FIXTURE_SEED)
    return _STATE[flavour]


def _handle(flavour):
    from lds import native
    if flavour not in _HANDLES:
        _HANDLES[flavour] = native.WavLM(_dims(flavour), _state(flavour))
    return _HANDLES[flavour]


def _clip(i):
    from lds import init_weights
    if i not in _CLIPS:
        _CLIPS[i] = wnp.make_clip(i, init_weights.uniform)
    return _CLIPS[i]


def _against(flavour, name, i, got, record_margin):
    z = fixtures()
    ref, rows = z[f"{flavour}_{name}_{i}"], z[f"{flavour}_rows_{i}"]
    assert got.shape == (wnp.FRAMES[i], ref.shape[1]), (got.shape, ref.shape)
    assert np.isfinite(got).all()
    e = relmax(got[rows], ref, float(z[f"{flavour}_absmax_{name}_{i}"]))
    print(f"{flavour} {name} clip {i}: max |native - ref64| / absmax {e:.3e} (the model's own fp32 gap {float(z[f'{flavour}_gap_{name}_{i}']):.2e})")
    record_margin(e, TOL, name)


@pytest.mark.parametrize("clip", range(len(wnp.CLIPS)))
@pytest.mark.parametrize("flavour", wnp.FLAVOURS)
def test_wavlm_vs_reference(flavour, clip, record_margin):
    """lds_wavlm_features and lds_wavlm_encode (hidden_states[1] and last_hidden_state) at full width with 2 layers, every recorded row of
    every fixture clip; the Large flavour normalises the raw clip on the device"""
    h, norm = _handle(flavour), flavour == "large"
    a = dev(_clip(clip)[None])
    _against(flavour, "feat", clip, h.features(a, normalize=norm)[0].cpu().numpy(), record_margin)
    _against(flavour, "h1", clip, h.encode(a, layer=1, normalize=norm)[0].cpu().numpy(), record_margin)
    _against(flavour, "last", clip, h.encode(a, normalize=norm)[0].cpu().numpy(), record_margin)


def test_wavlm_normalize_on_and_off(record_margin):
    """normalize = 0 on a waveform normalised by the caller gives what normalize = 1 gives on the raw one (both within TOL of the fixture:
    the caller's waveform is rounded to fp32 once more); on the raw waveform the two differ"""
    h = _handle("large")
    raw = dev(_clip(3)[None])
    pre = dev(wnp.normalize_wave(_clip(3), np.float32)[None])
    _against("large", "last", 3, h.encode(pre, normalize=False)[0].cpu().numpy(), record_margin)
    on, off = h.encode(raw, normalize=True), h.encode(raw, normalize=False)
    assert torch.isfinite(off).all() and float((on - off).abs().max()) > 1e-2
    b = _handle("base")      # the Base flavour takes the flag too: against the same handle on the caller's normalised waveform
    got, want = b.features(raw, normalize=True)[0].cpu().numpy(), b.features(pre, normalize=False)[0].cpu().numpy().astype(np.float64)
    record_margin(relmax(got, want) + 1e-30, TOL, "base.feat")


# ---- the gated-bias attention alone (include/lds_test.h lds_test_wavlm_attention) ----------------------------------------------------------
N_CTX = 1500


def _att_inputs(heads, T, B, tag):
    from lds import init_weights as iw
    C = 64 * heads
    qkv = iw.uniform(f"t.wavlm.att.{tag}.qkv", (B, 3 * C, T), 9, -1.0, 1.0)
    qkv[:, :2 * C] *= np.float32(1.7)      # logits of standard deviation ~ 3, as the encoder's
    gate = iw.uniform(f"t.wavlm.att.{tag}.gate", (B, heads, T), 9, 1.0, 2.0)
    gate[:, :, 0::3], gate[:, :, 1::3] = 1.0, 2.0      # both ends of the gate's range
    embed = iw.uniform(f"t.wavlm.att.{tag}.embed", (320, heads), 9, -2.0, 2.0)
    return qkv, gate, wnp.toeplitz(embed, 320, 800, N_CTX).astype(np.float32)


def _att_run(qkv, gate, toep, lens, n_ctx=N_CTX):
    from lds import native
    B, C3, T = qkv.shape
    heads = C3 // 192
    out = torch.full((B, C3 // 3, T), float("nan"), device="cuda")
    ln = None if lens is None else np.ascontiguousarray(lens, dtype=np.int32)
    d = [dev(v) for v in (qkv, gate, toep)]      # (kept alive over the call)
    native.check(native.lib().lds_test_wavlm_attention(native._dev(d[0]), native._dev(d[1]), native._dev(d[2]), native._host(ln), native._dev(out), B,
                                                       C3 // 3, T, heads, n_ctx, native._stream()))
    return out


def _att_ref(qkv, gate, toep, lens, n_ctx=N_CTX):
    """float64, one clip and one head at a time; zeros at and beyond a clip's length"""
    B, C3, T = qkv.shape
    heads = C3 // 192
    ref = np.zeros((B, C3 // 3, T))
    for b in range(B):
        n = T if lens is None else int(lens[b])
        x = qkv[b].astype(np.float64).reshape(3, heads, 64, T)[:, :, :, :n]
        for hd in range(heads):
            q, k, v = (np.ascontiguousarray(x[i, hd].T)[None] for i in range(3))
            o = wnp.biased_attention(q, k, v, gate[b, hd:hd + 1, :n].astype(np.float64), toep[hd:hd + 1].astype(np.float64), n_ctx)
            ref[b, hd * 64:(hd + 1) * 64, :n] = o[0].T
    return ref


@pytest.mark.parametrize("heads", [12, 16])
@pytest.mark.parametrize("T", [1, 31, 32, 33, 97, 350, 1500])
def test_biased_attention_alone(heads, T, record_margin):
    """every tile configuration (one wave; two key shares; four query tiles) and the sizes around their thresholds, gate values 1 and 2
    among them, against float64; distances up to 1499 reach both saturated buckets"""
    qkv, gate, toep = _att_inputs(heads, T, 1, f"{heads}.{T}")
    got = _att_run(qkv, gate, toep, None).cpu().numpy()
    assert np.isfinite(got).all()
    record_margin(relmax(got, _att_ref(qkv, gate, toep, None)), TOL)


@pytest.mark.parametrize("heads", [12, 16])
def test_biased_attention_mixed_lengths(heads, record_margin):
    """clips of 1500, 33 and 1 frames in one buffer, NaN in q, k, v and the gate beyond each: zeros beyond a clip, the float64 result inside;
    and a table of exactly 2 T - 1 entries (n_ctx = T)"""
    lens = (1500, 33, 1)
    qkv, gate, toep = _att_inputs(heads, 1500, 3, f"mix.{heads}")
    for b, n in enumerate(lens):
        qkv[b, :, n:] = np.nan
        gate[b, :, n:] = np.nan
    got = _att_run(qkv, gate, toep, lens).cpu().numpy()
    assert np.isfinite(got).all()
    for b, n in enumerate(lens):
        assert not got[b, :, n:].any()
    record_margin(relmax(got, _att_ref(np.nan_to_num(qkv), np.nan_to_num(gate), toep, lens)), TOL)
    q2, g2, _ = _att_inputs(heads, 97, 2, f"tight.{heads}")
    t2 = np.ascontiguousarray(toep[:, N_CTX - 97:N_CTX + 96])
    got2 = _att_run(q2, g2, t2, (97, 40), n_ctx=97).cpu().numpy()
    record_margin(relmax(got2, _att_ref(q2, g2, t2, (97, 40), n_ctx=97)), TOL, "n_ctx=T")


@pytest.mark.parametrize("heads,T,lens", [(12, 33, (33, 7)), (12, 97, (97, 32)), (16, 350, (350, 33)), (12, 1500, (1500, 1))])
def test_zero_table_equals_plain_attention_bit_for_bit(heads, T, lens):
    """the same kernel with an all-zero table against attention_k4p at D = 64 on the same inputs: the same tile rule and summation order,
    every score + 0"""
    from lds import native
    qkv, gate, toep = _att_inputs(heads, T, 2, f"zero.{heads}.{T}")
    got = _att_run(qkv, gate, np.zeros_like(toep), lens)
    plain = torch.full_like(got, float("nan"))
    d, ln = dev(qkv), np.ascontiguousarray(lens, dtype=np.int32)
    native.check(native.lib().lds_test_attention_ragged(native._dev(d), native._host(ln), native._dev(plain), 2, 64 * heads, T, heads, 0, 0, native._stream()))
    assert torch.isfinite(got).all() and torch.equal(got, plain)
    assert not torch.equal(_att_run(qkv, gate, toep, lens), plain)      # (and the table is not ignored)


# ---- ragged batches, poison, repeatability ---------------------------------------------------------------------------------------------------
def _ragged_audio(fill):
    a = np.full((3, max(RAGGED)), fill, dtype=np.float32)
    for b, (n, i) in enumerate(zip(RAGGED, (4, 4, 0))):
        a[b, :n] = _clip(i)[:n]
    return a


def _units_encoder(flavour, units_layer=None):
    from tools.tools import Units_Encoder, WavLMUnits
    name = "wavlmlarge" if flavour == "large" else "wavlmbase+"
    return Units_Encoder(name, model=WavLMUnits(name, dims=_dims(flavour), state=_state(flavour)), units_layer=units_layer)


@pytest.mark.parametrize("flavour", wnp.FLAVOURS)
def test_wavlm_encode_ragged_vs_alone(flavour, record_margin):
    """clips of 350, 3 and 1 frames as one Units_Encoder.encode_ragged, NaN beyond the clips: each against the clip alone (its own buffer
    length) within 1e-5 absmax, rows beyond T_b exactly zero"""
    enc = _units_encoder(flavour)
    assert enc.min_samples == 400 and enc.model.family == "WavLM" and enc.model.n_ctx == 1500
    audio = dev(_ragged_audio(np.nan))
    got, n_frames = enc.encode_ragged(audio, RAGGED)
    assert n_frames.tolist() == [350, 3, 1] and got.shape == (3, 350, _dims(flavour)["n_state"]) and torch.isfinite(got).all()
    worst = 0.0
    for b, n in enumerate(RAGGED):
        T = wnp.frames_of(n)
        alone = enc.encode(audio[b, :n].contiguous(), 16000)
        assert alone.shape == (T, got.shape[2])
        worst = max(worst, relmax(got[b, :T].cpu().numpy(), alone.cpu().numpy().astype(np.float64)))
        assert not got[b, T:].any(), b
    record_margin(worst + 1e-30, TOL_RAGGED)
    assert torch.equal(enc.encode(audio[0].contiguous(), 16000), _handle(flavour).encode(audio[:1].contiguous(), normalize=flavour == "large")[0])


@pytest.mark.parametrize("flavour", wnp.FLAVOURS)
def test_wavlm_poison_changes_nothing_and_repeats_are_identical(flavour):
    """NaN / 1e30 in the audio beyond lengths[b], a NaN / +Inf / -Inf workspace, repeated calls: bit-identical to the clean run"""
    from lds import native
    h, norm = _handle(flavour), flavour == "large"
    clean = dev(_ragged_audio(0.0))
    ref, ref_f = h.encode(clean, RAGGED, normalize=norm), h.features(clean, RAGGED, normalize=norm)
    assert torch.isfinite(ref).all() and torch.isfinite(ref_f).all()
    for fill in (np.nan, 1e30):
        bad = dev(_ragged_audio(fill))
        assert torch.equal(h.encode(bad, RAGGED, normalize=norm), ref) and torch.equal(h.features(bad, RAGGED, normalize=norm), ref_f), fill
    bad = dev(_ragged_audio(np.nan))
    ws = torch.empty(h.workspace_bytes(3, max(RAGGED)), dtype=torch.uint8, device="cuda")
    for pat in POISON:
        native.debug_fill(ws, pat)
        assert torch.equal(h.encode(bad, RAGGED, normalize=norm, ws=ws), ref), hex(pat)
        native.debug_fill(ws, pat)
        assert torch.equal(h.encode(bad, RAGGED, layer=1, normalize=norm, ws=ws), h.encode(clean, RAGGED, layer=1, normalize=norm)), hex(pat)
        native.debug_fill(ws, pat)
        assert torch.equal(h.features(bad, RAGGED, normalize=norm, ws=ws), ref_f), hex(pat)
    for _ in range(3):
        assert torch.equal(h.encode(bad, RAGGED, normalize=norm), ref)
    one = dev(_clip(3)[None])
    assert torch.equal(h.encode(one, normalize=norm), h.encode(one, normalize=norm))


def test_wavlm_units_layer_and_module_forward(record_margin):
    """Units_Encoder(units_layer=1) gives hidden_states[1]; the module's forward gives last_hidden_state and, asked, every hidden state"""
    from encoder.wavlm.model import WavLM
    enc = _units_encoder("base", units_layer=1)
    assert enc.model.units_layer == 1
    _against("base", "h1", 4, enc.encode(dev(_clip(4)), 16000).cpu().numpy(), record_margin)
    m = WavLM(_dims("large"), state=_state("large"))
    assert m.normalize
    o = m(dev(_clip(2)[None]), output_hidden_states=True)
    assert len(o.hidden_states) == 3 and torch.equal(o.hidden_states[2], o.last_hidden_state)
    _against("large", "h1", 2, o.hidden_states[1][0].cpu().numpy(), record_margin)
    _against("large", "last", 2, m(dev(_clip(2)[None])).last_hidden_state[0].cpu().numpy(), record_margin)


def test_wavlm_limits_return_their_codes_and_write_nothing():
    """every limit of a call: LDS_EINVAL (-1) with a message, LDS_ENOMEM (-2) naming the size, and the output still holds its sentinel"""
    from lds import native
    h = _handle("base")
    L = native.lib()
    audio = dev(_clip(1)[None].repeat(2, 0))      # [2][720]: 2 frames
    out = torch.full((2, 2, 768), 7.0, device="cuda")
    nbytes = h.workspace_bytes(2, 720)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    big = torch.zeros(1, 480400, device="cuda")      # 1501 frames

    def enc(a=audio, lens=None, layer=2, norm=0, w=ws, wb=None, B=2, n=720):
        ln = None if lens is None else np.ascontiguousarray(lens, dtype=np.int32)
        rc = L.lds_wavlm_encode(h.h, native._dev(a), native._host(ln), native._dev(out), layer, norm, native._dev(w), w.numel() if wb is None else wb, B, n,
                                native._stream())
        return rc, L.lds_last_error().decode()

    for kw, code, word in ((dict(B=65), -1, "B 65"), (dict(B=0), -1, "B 0"), (dict(n=399), -1, "399"), (dict(a=big, B=1, n=480400), -1, "exceed n_ctx"),
                           (dict(layer=3), -1, "n_layers_run 3"), (dict(layer=-1), -1, "n_layers_run -1"), (dict(norm=2), -1, "normalize 2"),
                           (dict(lens=[720, 399]), -1, "length[1] = 399"), (dict(lens=[721, 720]), -1, "length[0] = 721"),
                           (dict(wb=nbytes - 1), -2, f"need {nbytes}")):
        rc, msg = enc(**kw)
        assert rc == code and word in msg, (kw, rc, msg)
    assert L.lds_wavlm_features(h.h, native._dev(audio), None, native._dev(out), 2, native._dev(ws), ws.numel(), 2, 720, native._stream()) == -1
    assert L.lds_wavlm_encode(h.h, None, None, native._dev(out), 2, 0, native._dev(ws), ws.numel(), 2, 720, native._stream()) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert enc() [0] == 0      # (the same arguments without a fault run)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and not bool((out == 7.0).all())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        h.encode(torch.zeros(1, 16000))


def test_wavlm_end_to_end_infer_svc(tmp_path):
    """infer_svc.py --synthetic --encoder wavlmbase+: Units_Encoder('wavlmbase+') feeds Unit2Mel and the vocoder through
    DiffusionSVC.infer_from_long_audio"""
    import infer_svc
    from tools.tools import get_encdoer_out_channels
    out = str(tmp_path / "out.npy")
    wav = infer_svc.main(["--synthetic", "--encoder", "wavlmbase+", "--synthetic_layers", "2", "--synthetic_seconds", "4", "-o", out, "-s", "100"])
    assert wav.ndim == 1 and wav.shape[0] > 44100 and np.isfinite(wav).all() and float(np.abs(wav).max()) > 0
    assert np.array_equal(np.load(out), wav) and get_encdoer_out_channels("wavlmbase+") == 768
