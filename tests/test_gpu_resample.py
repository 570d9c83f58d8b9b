"""The polyphase resampler on the GPU (tools.tools.Resample, include/lds.h lds_resample / lds_resample_ragged): every output against the
float64 closed form evaluated with the library's fp32 bank (tests/resample_numpy.py apply_bank64), within the a-priori bound of an fp32
dot product; the ragged form's bit-exact guarantees; the opt-in wiring into Units_Encoder, Vocoder and tools/extract_units.py.

The bound (derived, not measured): the kernel computes each output as one fp32 fmaf chain over the T taps of its phase.  For any
summation order, with or without FMA, |computed - exact| <= gamma_{T+1} sum_n |x[n]| |g_n| with gamma_k = k u / (1 - k u), u = 2^-24
(Higham, Accuracy and Stability of Numerical Algorithms, section 3.1; the products are exact under FMA, so T roundings at most).  At
441:160 (34 taps, sum |g| ~ 1.6) that is about 4e-6 max |x|.  The reference values are float64 sums of the same fp32 taps: their own
error, 34 x 2^-53, is nine orders below."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

import resample_numpy as RN
from conftest import ROOT

pytestmark = pytest.mark.gpu

# (orig, new, lowpass_filter_width, rolloff): the six common pairs, then the shapes at which the launcher takes another path
PAIRS = [
    (44100, 16000, 6, 0.99),      # 441:160, bank in LDS (160 x 34), 2048 outputs per workgroup
    (16000, 44100, 6, 0.99),      # 160:441, bank in LDS (441 x 13)
    (48000, 16000, 6, 0.99),      # one phase
    (22050, 44100, 6, 0.99),      # O = 1
    (44100, 48000, 6, 0.99),
    (16000, 44101, 6, 0.99),      # 44,101 phases x 13 taps: the bank stays in global memory
    (48000, 8000, 6, 0.99),       # 6:1, 73 taps: the input span of 2048 outputs does not fit, 1024 per workgroup
    (44100, 16000, 16, 0.95),     # another width and rolloff: 160 x 94 entries, read from global memory
    (40000, 100, 1, 0.99),        # 400:1 behind a narrow filter (809 taps): 64 outputs need 26,000 samples, the one-thread-per-output kernel
]


def _lengths(O):
    return sorted({n for n in (1, 7, O - 1, O, O + 1, 4410, 100003) if n >= 1})


def _signals(L, seed):
    rng = np.random.default_rng(seed)
    sq = np.where((np.arange(L) // 37) % 2 == 0, 1.0, -1.0).astype(np.float32)      # full-scale +-1 square wave
    return np.stack([rng.standard_normal(L).astype(np.float32), sq])


def _worst_ratio(got, x, t, lengths=None):
    """max over the batch of |got - float64 reference| / bound; asserts the shape and the zeros beyond every clip's own output"""
    worst = 0.0
    for b in range(x.shape[0]):
        ref, bound = RN.apply_bank64(x[b], t["O"], t["N"], t["bankT"], t["first"], None if lengths is None else lengths[b])
        err = np.abs(got[b, :len(ref)].astype(np.float64) - ref)
        assert (err <= bound).all(), (b, float(err.max()), float(bound[np.argmax(err - bound)]))
        assert not got[b, len(ref):].any()
        if len(ref):
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    return worst


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}to{p[1]}w{p[2]}")
def test_resample_against_float64_closed_form(pair, record_margin):
    import torch
    from lds import native
    from tools.tools import Resample
    orig, new, w, rolloff = pair
    rs = Resample(orig, new, lowpass_filter_width=w, rolloff=rolloff).to("cuda")
    t = native.resample_tables(orig, new, w, rolloff)
    worst = 0.0
    for L in _lengths(t["O"]):
        x = _signals(L, L)
        got = rs(torch.from_numpy(x).cuda())
        assert got.shape == (2, RN.out_length(L, t["O"], t["N"])) and got.dtype == torch.float32 and got.is_cuda
        ratio = _worst_ratio(got.cpu().numpy(), x, t)
        print(f"{orig}->{new} L {L}: worst err / bound {ratio:.3f}")
        worst = max(worst, ratio)
    record_margin(worst, 1.0)


def test_resample_30s_clip_64bit_indices_and_leading_dims(record_margin):
    """1,323,000 samples (30 s at 44.1 kHz), 235 workgroups per clip; the [2, 1, L] input keeps its leading dimensions as torchaudio's
    transform does.  (The products that pass 2^31 are in the 16000 -> 44101 case above: m O = 275,640 x 16,000.)"""
    import torch
    from lds import native
    from tools.tools import Resample
    L = 1323000
    x = _signals(L, 5)
    t = native.resample_tables(44100, 16000)
    got = Resample(44100, 16000)(torch.from_numpy(x).cuda().reshape(2, 1, L))
    assert got.shape == (2, 1, 480000)
    record_margin(_worst_ratio(got.reshape(2, -1).cpu().numpy(), x, t), 1.0)
    same = Resample(16000, 16000)
    a = torch.zeros(3, device="cuda")
    assert same(a) is a


RAGGED = [(44100, 16000), (16000, 44100), (16000, 44101), (40000, 100)]


@pytest.mark.parametrize("pair", RAGGED, ids=lambda p: f"{p[0]}to{p[1]}")
def test_ragged_is_every_clip_alone_bit_for_bit(pair, record_margin):
    import torch
    from lds import native
    from tools.tools import Resample
    orig, new = pair
    w = 1 if orig == 40000 else 6
    rs = Resample(orig, new, lowpass_filter_width=w)
    t = native.resample_tables(orig, new, w)
    L = 120000
    lens = [L, 1, 441, 100003, 17761]
    rng = np.random.default_rng(11)
    x = rng.standard_normal((5, L)).astype(np.float32)
    mask = np.arange(L)[None, :] >= np.asarray(lens)[:, None]
    outs = []
    for fill in (0.0, np.nan, 1e30):
        xf = np.where(mask, np.float32(fill), x)
        y, nl = rs.forward_ragged(torch.from_numpy(xf).cuda(), lens)
        outs.append(y.cpu().numpy())
        assert nl.dtype == torch.int64 and not nl.is_cuda and nl.tolist() == [RN.out_length(n, t["O"], t["N"]) for n in lens]
        assert y.shape == (5, max(nl.tolist()))
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])      # nothing beyond lengths[b] reaches a result
    record_margin(_worst_ratio(outs[1], x, t, lens), 1.0)                            # (and zeros beyond each clip's own output)
    xd = torch.from_numpy(x).cuda()
    for b, n in enumerate(lens):                                                     # every clip = the clip resampled alone
        alone = rs(xd[b, :n].clone()).cpu().numpy()
        assert np.array_equal(outs[0][b, :len(alone)], alone), b
    for _ in range(5):                                                               # repeats are bit-identical
        assert np.array_equal(rs.forward_ragged(torch.from_numpy(np.where(mask, np.float32(np.nan), x)).cuda(), lens)[0].cpu().numpy(), outs[0])
    yd = rs(xd)                                                                      # all lengths L = the dense entry
    yr, nl = rs.forward_ragged(xd, [L] * 5)
    assert torch.equal(yd, yr) and nl.tolist() == [yd.shape[1]] * 5
    # a batch of its own permutation: a clip's bits do not depend on its row
    perm = [3, 0, 4, 2, 1]
    yp, _ = rs.forward_ragged(torch.from_numpy(np.where(mask, np.float32(0), x)[perm]).cuda(), [lens[p] for p in perm])
    assert np.array_equal(yp.cpu().numpy(), outs[0][perm])


def test_ragged_zero_length_clip_and_limits():
    import torch
    from tools.tools import Resample
    rs = Resample(44100, 16000)
    x = torch.full((2, 1000), float("nan"), device="cuda")
    x[1, :500] = 1.0
    y, nl = rs.forward_ragged(x, [0, 500])
    assert nl.tolist() == [0, 182] and y.shape == (2, 182) and not y[0].any() and torch.isfinite(y).all()
    with pytest.raises(ValueError, match="lengths"):
        rs.forward_ragged(x, [0, 1001])
    with pytest.raises(ValueError, match="at most 64"):
        rs.forward_ragged(torch.zeros(65, 8, device="cuda"), [8] * 65)


# ---- wiring ----------------------------------------------------------------------------------------------------------------------------
def _small_whisper():
    from encoder.whisper.model import ModelDimensions
    from lds import arch
    from tools.tools import WhisperLargeV3
    return WhisperLargeV3.synthetic(ModelDimensions(**dict(arch.WHISPER_LARGE_V3_DIMS, n_audio_state=128, n_audio_head=2, n_audio_layer=1)), device="cuda")


def test_units_encoder_resamples_by_opt_in():
    import torch
    from tools.tools import Resample, Units_Encoder
    model = _small_whisper()
    on = Units_Encoder("whisper_large_v3", device="cuda", model=model, resample=True)
    off = Units_Encoder("whisper_large_v3", device="cuda", model=model)
    rng = np.random.default_rng(3)
    a44 = torch.from_numpy((0.1 * rng.standard_normal(50000)).astype(np.float32)).cuda()
    rs = Resample(44100, 16000)
    want = off.encode(rs(a44), 16000)
    got = on.encode(a44, 44100)
    assert got.shape == want.shape and torch.equal(got, want) and list(on.resample_kernel) == ["44100"]
    assert torch.equal(on.encode(a44[:900], 44100), off.encode(rs(a44[:900]), 16000))      # 327 samples at 16 kHz: padded to 400
    with pytest.raises(ValueError, match="44100.*16000.*resample=True"):
        off.encode(a44, 44100)
    # ragged: lengths at 44.1 kHz in, n_frames from the resampled lengths
    lens = [50000, 1200, 33075]
    batch = torch.full((3, 50000), float("nan"), device="cuda")
    for b, n in enumerate(lens):
        batch[b, :n] = a44[:n]
    units, n_frames = on.encode_ragged(batch, lens, 44100)
    r16, l16 = rs.forward_ragged(batch, lens)
    assert l16.tolist() == [18141, 436, 12000]
    want_u, want_f = off.encode_ragged(r16, l16)
    assert torch.equal(units, want_u) and n_frames.tolist() == want_f.tolist() == [(n // 160 - 1) // 2 + 1 for n in l16.tolist()]
    with pytest.raises(ValueError, match="44100.*16000"):
        off.encode_ragged(batch, lens, 44100)


def test_vocoder_extract_resamples_by_opt_in():
    import torch
    from diffusion.vocoder import Vocoder
    from encoder.hifi_vaegan.hifi_vaegan import Hifi_VAEGAN
    from lds import arch, init_weights
    from tools.tools import Resample
    h = arch.SYNTHETIC_VOCODER_H
    voc = Vocoder.__new__(Vocoder)      # (no checkpoint ships: the wrapper around a seeded encoder, as the encoder's own tests build it)
    voc.vocoder = Hifi_VAEGAN(None, device="cuda", h=h, state={}, encoder_state=init_weights.init_state(arch.encoder_param_shapes(h), 0))
    voc.vocoder_sample_rate, voc.vocoder_hop_size, voc.dimension = 44100, 512, 80
    rng = np.random.default_rng(4)
    a = torch.from_numpy((0.3 * rng.standard_normal((2, 3000))).astype(np.float32)).cuda()
    rs = Resample(22050, 44100)
    with pytest.raises(ValueError, match="22050.*44100.*resample=True"):
        voc.extract(a, 22050)
    with pytest.raises(ValueError, match="22050.*44100"):
        voc.extract_ragged(a, 22050, [3000, 1000])
    voc.resample = True
    torch.manual_seed(9)
    got = voc.extract(a, 22050)
    torch.manual_seed(9)
    want = voc.extract(rs(a), 44100)
    assert got.shape == (2, 12, 160) and torch.equal(got, want) and list(voc.resample_kernel) == ["22050"]
    torch.manual_seed(9)
    got_r = voc.extract_ragged(a, 22050, [3000, 1000], only_mean=True)
    torch.manual_seed(9)
    r44, l44 = rs.forward_ragged(a, [3000, 1000])
    assert l44.tolist() == [6000, 2000] and torch.equal(got_r, voc.extract_ragged(r44, 44100, l44, only_mean=True))


def _write_wav(path, pcm, rate):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(pcm.tobytes())


def test_extract_units_tool_resamples_wav_clips(tmp_path):
    """three 44.1 kHz PCM16 .wav clips through the tool = the clips resampled with Resample, saved as 16 kHz .npy, through the tool"""
    import torch
    from tools.tools import Resample
    rng = np.random.default_rng(8)
    wdir, ndir = tmp_path / "wav", tmp_path / "npy"
    wdir.mkdir()
    ndir.mkdir()
    rs = Resample(44100, 16000)
    for i, n in enumerate((30000, 700, 44100)):      # (700 samples: 254 at 16 kHz, zero-padded to 400 by the tool)
        pcm = (rng.standard_normal(n) * 3000).astype(np.int16)
        _write_wav(wdir / f"c{i}.wav", pcm, 44100)
        np.save(ndir / f"c{i}.npy", rs(torch.from_numpy(pcm.astype(np.float32) / 32768.0).cuda()).cpu().numpy())
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    for d in (wdir, ndir):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "extract_units.py"), str(d), "--out", str(d / "units"), "--synthetic", "--layers", "2"],
                           capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    for i, n16 in enumerate((10885, 400, 16000)):
        a, b = np.load(wdir / "units" / f"c{i}.npy"), np.load(ndir / "units" / f"c{i}.npy")
        assert a.shape == ((n16 // 160 - 1) // 2 + 1, 1280) and np.array_equal(a, b), i
