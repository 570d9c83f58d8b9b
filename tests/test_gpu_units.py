"""The Whisper units encoder on the GPU (include/lds.h lds_whisper_*, tools.tools.Units_Encoder): the log-mel front end and the encoder
against the fixtures recorded from the reference, the full-width model against the numpy restatement (tests/whisper_numpy.py, pinned to
the same fixtures by tests/test_cpu_units.py), and the ragged-batch invariants."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import whisper_numpy as wnp
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

TOL = 2e-5              # x absmax: the project's bound for an fp32 forward against the reference (the UNet's; same kernels, same op classes)
TOL_RAGGED = 1e-5       # x absmax: a clip inside a ragged batch against the clip alone (the VAE encoder's bound)
POISON = (0x7FC00000, 0x7F800000, 0xFF800000)      # NaN, +Inf, -Inf


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def relmax(got, ref):
    return float(np.abs(got.astype(np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


def _filters(n_mels):
    return np.load(os.path.join(GOLDEN, "whisper_mel_filters.npz"))[f"mel_{n_mels}"]


_HANDLES = {}


def _handle(n_mels, C, heads, layers, n_ctx=1500):
    from lds import arch, native
    key = (n_mels, C, heads, layers, n_ctx)
    if key not in _HANDLES:
        _HANDLES[key] = native.Whisper(n_mels, C, heads, layers, n_ctx, arch.whisper_init_state(n_mels, C, layers, 0), arch.whisper_mel_filters(n_mels))
    return _HANDLES[key]


def _clip(z, i):
    from lds import init_weights
    return wnp.make_signal(f"clip{i}", int(z[f"n_{i}"]), int(z[f"seed_{i}"]), init_weights.uniform, bool(z[f"quiet_{i}"]))


@pytest.mark.parametrize("n_mels", [128, 80])
@pytest.mark.parametrize("clip", [0, 1, 2, 3, 4])
def test_units_logmel_vs_reference(clip, n_mels, record_margin):
    """every element of every fixture clip: max |native - reference fp64| <= 2 x E_ref, E_ref = max |reference fp32 - reference fp64| of that
    clip (the allowance for a different but equally long fp32 evaluation; the fixture stores the fp64 result rounded to fp32, 6e-8).
    Through lds_whisper_logmel and through encoder.whisper.audio.log_mel_spectrogram (same bits)."""
    from encoder.whisper.audio import log_mel_spectrogram
    z = np.load(os.path.join(GOLDEN, f"whisper_logmel_{n_mels}.npz"))
    audio = _clip(z, clip)
    ref, eref = z[f"ref64_{clip}"].astype(np.float64), float(z[f"eref_{clip}"])
    got = _handle(n_mels, 128, 2, 1).logmel(dev(audio[None]))[0]
    py = log_mel_spectrogram(dev(audio), n_mels=n_mels)
    assert py.shape == ref.shape and torch.equal(py, got)
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max())
    print(f"logmel n_mels {n_mels} clip {clip}: max |native - ref64| {err:.3e}, E_ref {eref:.3e}, measured / bound {err / (2 * eref):.3f}")
    record_margin(err, 2 * eref)


@pytest.mark.parametrize("name", ["a", "b"])
def test_units_encoder_vs_reference(name, record_margin):
    """AudioEncoder.forward from the fixture's mel (lds_whisper_encode_mel, and the same through encoder.whisper.model.AudioEncoder)"""
    from encoder.whisper.model import ModelDimensions, Whisper
    from lds import arch, init_weights
    z = np.load(os.path.join(GOLDEN, "whisper_encoder.npz"))
    n_mels, C, H, layers, F, seed = (int(v) for v in z[name + "_dims"])
    mel = dev(init_weights.uniform(f"fix.whisper.{name}.mel", (1, n_mels, F), seed, -1.0, 1.5))
    got = _handle(n_mels, C, H, layers).encode_mel(mel)
    ref = z[name + "_out"]
    assert tuple(got.shape) == ref.shape
    model = Whisper(ModelDimensions(**dict(arch.WHISPER_LARGE_V3_DIMS, n_mels=n_mels, n_audio_state=C, n_audio_head=H, n_audio_layer=layers)))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in arch.whisper_init_state(n_mels, C, layers, 0).items()})
    assert torch.equal(model.encoder(mel), got) and torch.equal(model.embed_audio(mel), got)
    err = relmax(got.cpu().numpy(), ref)
    print(f"encoder {name}: {err:.3e} (the reference's own fp32-vs-fp64 gap {float(z[name + '_gap']):.2e})")
    record_margin(err, TOL)


def _units_encoder(dims_kw):
    from encoder.whisper.model import ModelDimensions
    from lds import arch
    from tools.tools import Units_Encoder, WhisperLargeV3
    dims = ModelDimensions(**dict(arch.WHISPER_LARGE_V3_DIMS, **dims_kw))
    return Units_Encoder("whisper_large_v3", device="cuda", model=WhisperLargeV3.synthetic(dims, seed=0, device="cuda"))


def test_units_end_to_end_vs_reference(record_margin):
    """the body of WhisperLargeV3.__call__ (log-mel, encoder, squeeze) through lds_whisper_encode and through Units_Encoder.encode"""
    from lds import init_weights
    z = np.load(os.path.join(GOLDEN, "whisper_encoder.npz"))
    audio = dev(wnp.make_signal("e2e", int(z["e2e_n"]), int(z["e2e_seed"]), init_weights.uniform, False))
    got = _handle(128, 128, 2, 4).encode(audio[None])[0]
    ue = _units_encoder(dict(n_audio_state=128, n_audio_head=2, n_audio_layer=4))
    py = ue.encode(audio, 16000)
    assert py.is_cuda and tuple(py.shape) == z["e2e_out"].shape and torch.equal(py, got)
    assert torch.equal(ue.encode(audio[None], 16000), got)      # [1, L] as the reference's callers pass it
    err = relmax(got.cpu().numpy(), z["e2e_out"])
    print(f"end to end: {err:.3e} (the reference's own fp32-vs-fp64 gap {float(z['e2e_gap']):.2e}, x {err / float(z['e2e_gap']):.1f})")
    record_margin(err, TOL)


def test_units_short_clip_is_padded_to_400_samples():
    ue = _units_encoder(dict(n_audio_state=128, n_audio_head=2, n_audio_layer=4))
    from lds import init_weights
    a = dev(init_weights.uniform("short.audio", (250,), 5, -0.5, 0.5))
    got = ue.encode(a, 16000)
    assert tuple(got.shape) == (1, 128)      # 400 samples: 2 mel frames, 1 encoder frame
    assert torch.equal(got, ue.encode(torch.nn.functional.pad(a, (0, 150)), 16000))


FULL = dict(n_mels=128, C=1280, heads=20, layers=4)
FULL_LENS = [480000, 112077, 400]
_FULL_REF = {}


def _full_audio():
    from lds import init_weights
    a = np.zeros((3, 480000), dtype=np.float32)
    for b, n in enumerate(FULL_LENS):
        a[b, :n] = wnp.make_signal(f"full{b}", n, 51 + b, init_weights.uniform, quiet_second_half=(b == 1))
    return a


def _full_ref(b):
    """tests/whisper_numpy.py in fp32 for clip b of the full-width case (computed once per session)"""
    from lds import arch
    if b not in _FULL_REF:
        w = arch.whisper_init_state(FULL["n_mels"], FULL["C"], FULL["layers"], 0)
        _FULL_REF[b] = wnp.encode(w, _full_audio()[b, :FULL_LENS[b]], _filters(128), FULL["heads"], np.float32)
    return _FULL_REF[b]


def test_units_full_width_one_30s_clip(record_margin):
    """n_state 1280, 20 heads, n_mels 128, 4 layers (every shape and tile of the 32-layer model), one clip of 1500 frames"""
    h = _handle(FULL["n_mels"], FULL["C"], FULL["heads"], FULL["layers"])
    got = h.encode(dev(_full_audio()[:1]))
    assert tuple(got.shape) == (1, 1500, 1280) and torch.isfinite(got).all()
    _FULL_REF["native0"] = got[0].cpu()
    err = relmax(got[0].cpu().numpy(), _full_ref(0))
    print(f"full width, 1500 frames: {err:.3e}")
    record_margin(err, TOL)


def test_units_full_width_ragged_batch(record_margin):
    """B = 3 with lengths 480,000 / 112,077 / 400 through Units_Encoder.encode_ragged: every clip against the restatement of the clip alone"""
    ue = _units_encoder(dict(n_audio_layer=FULL["layers"]))
    units, n_frames = ue.encode_ragged(dev(_full_audio()), FULL_LENS)
    assert tuple(units.shape) == (3, 1500, 1280) and n_frames.tolist() == [1500, 350, 1] and torch.isfinite(units).all()
    if "native0" in _FULL_REF:      # the 30 s clip alone (the test above) and as the first of three: the same bits
        assert torch.equal(units[0].cpu(), _FULL_REF["native0"])
    units = units.cpu().numpy()
    worst = 0.0
    for b, T in enumerate(n_frames.tolist()):
        ref = _full_ref(b)
        assert ref.shape == (T, 1280)
        e = relmax(units[b, :T], ref)
        print(f"full width ragged, clip {b} ({FULL_LENS[b]} samples, {T} frames): {e:.3e}")
        worst = max(worst, e)
        assert not units[b, T:].any(), b
    record_margin(worst, TOL)
    # ... and against the native encode of the clip alone, in a buffer of its own length (other tiles, other rounding)
    h = _handle(FULL["n_mels"], FULL["C"], FULL["heads"], FULL["layers"])
    alone = h.encode(dev(_full_audio()[1:2, :FULL_LENS[1]]))[0].cpu().numpy()
    e = relmax(units[1, :350], alone.astype(np.float64))
    print(f"full width ragged, clip 1 against its stand-alone encode: {e:.3e}")
    record_margin(e, TOL_RAGGED, "alone")


# ---- ragged invariants (DESIGN 16's set) on a small model: one buffer of 48,000 samples ----
SMALL = (128, 128, 2, 4)
LENS = [48000, 400, 31999, 17761, 24000]      # the full buffer, the shortest clip, odd frame counts, a length 160 does not divide


def _ragged_audio(fill):
    from lds import init_weights
    a = np.zeros((len(LENS), 48000), dtype=np.float32)
    for b, n in enumerate(LENS):
        a[b, :n] = wnp.make_signal(f"rg{b}", n, 61 + b, init_weights.uniform, quiet_second_half=(b == 2))
        a[b, n:] = fill
    return a


def test_units_ragged_vs_alone(record_margin):
    """every clip of a ragged batch against the same clip encoded alone (NaN beyond the clips); rows beyond T_b exactly zero"""
    h = _handle(*SMALL)
    audio = dev(_ragged_audio(np.nan))
    got = h.encode(audio, LENS)
    mel = h.logmel(audio, LENS)
    assert tuple(got.shape) == (5, 150, 128) and torch.isfinite(got).all() and torch.isfinite(mel).all()
    worst = 0.0
    for b, n in enumerate(LENS):
        F, T = wnp.frames_of(n)
        alone = h.encode(audio[b:b + 1, :n].contiguous())[0]
        worst = max(worst, relmax(got[b, :T].cpu().numpy(), alone.cpu().numpy().astype(np.float64)))
        assert not got[b, T:].any() and not mel[b, :, F:].any(), b
        assert torch.equal(mel[b, :, :F], h.logmel(audio[b:b + 1, :n].contiguous())[0]), b      # the front end has no tile choice: same bits
    record_margin(worst, TOL_RAGGED)


def test_units_padding_contents_are_irrelevant():
    """NaN, 1e30 and zeros beyond lengths[b] give bit-identical units and log-mels"""
    h = _handle(*SMALL)
    outs = [(h.encode(dev(_ragged_audio(f)), LENS), h.logmel(dev(_ragged_audio(f)), LENS)) for f in (0.0, np.nan, 1e30)]
    for u, m in outs[1:]:
        assert torch.equal(u, outs[0][0]) and torch.equal(m, outs[0][1])


def test_units_poisoned_workspace_changes_nothing():
    from lds import native
    h = _handle(*SMALL)
    audio = dev(_ragged_audio(np.nan))
    ref = h.encode(audio, LENS)
    ref_mel = h.logmel(audio, LENS)
    ws = torch.empty(h.workspace_bytes(5, 48000), dtype=torch.uint8, device="cuda")
    for pat in POISON:
        native.debug_fill(ws, pat)
        assert torch.equal(h.encode(audio, LENS, ws=ws), ref), hex(pat)
        native.debug_fill(ws, pat)
        assert torch.equal(h.logmel(audio, LENS, ws=ws), ref_mel), hex(pat)
        native.debug_fill(ws, pat)
        assert torch.equal(h.encode(audio[:1].contiguous(), ws=ws), h.encode(audio[:1].contiguous())), hex(pat)


def test_units_all_full_lengths_is_the_plain_call_bit_for_bit():
    from lds import init_weights
    h = _handle(*SMALL)
    audio = dev(np.stack([wnp.make_signal(f"eq{b}", 48000, 71 + b, init_weights.uniform) for b in range(3)]))
    assert torch.equal(h.encode(audio, [48000] * 3), h.encode(audio))
    assert torch.equal(h.logmel(audio, [48000] * 3), h.logmel(audio))
    mel = h.logmel(audio)
    assert torch.equal(h.encode_mel(mel, [300] * 3), h.encode_mel(mel))
    assert torch.equal(h.encode_mel(mel), h.encode(audio))      # the split entries compose to the fused one


def test_units_repeated_calls_are_bit_identical():
    h = _handle(*SMALL)
    audio = dev(_ragged_audio(0.0))
    first = h.encode(audio, LENS)
    for _ in range(4):
        assert torch.equal(h.encode(audio, LENS), first)


def test_units_a_clip_does_not_depend_on_its_batch():
    """the tile rules are judged at the nominal batch: the same clip gives the same bits alone, first of three and last of five"""
    from lds import init_weights
    h = _handle(*SMALL)
    a = np.stack([wnp.make_signal(f"bi{b}", 48000, 81 + b, init_weights.uniform) for b in range(5)])
    alone = h.encode(dev(a[:1]))
    assert torch.equal(h.encode(dev(a[:3]))[0], alone[0])
    assert torch.equal(h.encode(dev(a[::-1].copy()))[4], alone[0])


def test_extract_units_tool_synthetic(tmp_path):
    """tools/extract_units.py --synthetic on three generated clips writes three .npy files of the right shapes"""
    from lds import init_weights
    lens = [16000, 5000, 23456]
    for i, n in enumerate(lens):
        np.save(tmp_path / f"clip{i}.npy", wnp.make_signal(f"tool{i}", n, 91 + i, init_weights.uniform))
    out = tmp_path / "units"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "extract_units.py"), str(tmp_path), "--out", str(out), "--synthetic", "--layers", "2",
                        "--batch", "2"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for i, n in enumerate(lens):
        u = np.load(out / f"clip{i}.npy")
        assert u.shape == (wnp.frames_of(n)[1], 1280) and u.dtype == np.float32 and np.isfinite(u).all() and np.abs(u).max() > 0.1
