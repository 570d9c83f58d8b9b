"""The vocoder's log-mel analysis on the GPU (csrc/stftmel.hip through STFT.get_mel / Hifi_VAEGAN.get_mel): every fixture clip and keyshift
against the reference's lines in float64 within twice the reference's own fp32 error, the f64 MFMA's fragment map on exact integers, the
padding modes and frame counts at the edges, a ragged batch against every clip alone whatever the buffer holds beyond the clips, and
repeatability."""
import numpy as np
import pytest
import torch

import stftmel_numpy as SN

pytestmark = pytest.mark.gpu

# fp32 tail on an exact DFT: a sequential sum of at most 64 non-negative products (gamma_64), the magnitude's three roundings and the
# scale's two, in the log domain where a relative error is an absolute one, plus the result's own rounding (|log| < 16): 70 * 2^-24 + 2^-20
TAIL_TOL = 70 * 2.0 ** -24 + 2.0 ** -20


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def stft():
    from encoder.hifi_vaegan.modules.nvSTFT import STFT
    return STFT(SN.SR, SN.N_MELS, SN.N_FFT, SN.WIN, SN.HOP, SN.FMIN, SN.FMAX)


@pytest.fixture(scope="module")
def fx(golden):
    return golden("vocoder_mel.npz")


def ref64(clip, keyshift=0, speed=1):
    from lds import stftmel
    win_new = SN.geometry(keyshift, speed)[1]
    bank = stftmel.slaney_mel(SN.SR, SN.N_FFT, SN.N_MELS, SN.FMIN, SN.FMAX)
    return SN.get_mel64(clip, torch.hann_window(win_new).numpy(), bank, keyshift=keyshift, speed=speed)


@pytest.mark.parametrize("k", SN.KEYSHIFTS)
@pytest.mark.parametrize("i", range(len(SN.CLIPS)))
def test_mel_vs_reference(stft, fx, i, k, record_margin):
    """max |native - ref64| <= 2 x eref in the log domain over every element: eref = the reference's own fp32 run against the same float64
    evaluation (the bound of test_units_logmel_vs_reference)"""
    ref, eref = fx[f"ref64_{i}_{k}"], float(fx[f"eref_{i}_{k}"])
    got = stft.get_mel(dev(fx[f"clip_{i}"])[None], keyshift=k)
    assert tuple(got.shape) == (1,) + ref.shape and got.dtype == torch.float32
    got = got[0].cpu().numpy()
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"clip {i} keyshift {k}: err {err:.3e}, eref {eref:.3e}, ratio {err / eref:.2f}")
    floor = np.log(np.float64(np.float32(SN.CLIP)))
    dead = ref == floor
    assert dead.any() == (k < 0) and (got[dead] == np.float32(floor)).all()      # rows of zeroed bins only: exactly log(clip_val)
    record_margin(err, 2 * eref)


def test_hifi_vaegan_get_mel_is_the_same_bits_transposed(stft, fx):
    from encoder.hifi_vaegan.hifi_vaegan import Hifi_VAEGAN
    from lds import arch
    v = Hifi_VAEGAN(None, device="cuda", h=arch.SYNTHETIC_VOCODER_H, state={})
    x = dev(np.stack([fx["clip_0"], fx["clip_4"]]))
    for k in (0, -7):
        a, b = v.get_mel(x, keyshift=k), stft.get_mel(x, keyshift=k)
        assert tuple(a.shape) == (2, SN.frames(3072, k), 128) and torch.equal(a, b.transpose(1, 2))


@pytest.mark.parametrize("n", [64, 70])
def test_fragment_map_on_exact_integers(n):
    """an asymmetric integer basis times integer audio: every product and sum is exact in double, so any row / column swap of the f64 MFMA's
    operand or C/D map changes the result; 70 is no multiple of the K step of 4, 33 / 36 bins no multiple of the tile of 16"""
    from lds import native
    hop, F, B = 16, 5, 2
    L, bins = n + hop * (F - 1), n // 2 + 1
    rng = np.random.RandomState(7)
    audio = rng.randint(-8, 9, size=(B, L)).astype(np.float32)
    nn, kk = np.arange(n)[:, None], np.arange(bins)[None, :]
    basis = np.stack([(3 * nn + 5 * kk + nn * kk) % 7 - 3, (2 * nn + 7 * kk + 3 * nn * kk) % 11 - 5], axis=-1).astype(np.float64)
    melT = rng.uniform(0, 1, size=(bins, 128)).astype(np.float32)
    got = native.stft_dft_probe(dev(audio), dev(basis), dev(melT), n, hop)
    frames = np.stack([audio[:, f * hop:f * hop + n] for f in range(F)], axis=1).astype(np.float64)      # [B, F, n]
    ref = np.einsum("bfn,nkc->bfkc", frames, basis)
    assert tuple(got.shape) == ref.shape == (B, F, bins, 2)
    assert torch.equal(got.cpu(), torch.from_numpy(ref))


@pytest.mark.parametrize("L,keyshift,speed", [(700, 0, 1), (1500, 0, 1), (2048 - 768, 0, 1), (768, 0, 1), (769, 0, 1), (512 * 3 + 137, 0, 1),
                                              (512 * 40 + 137, 0, 1), (3209, 0, 2), (684, -7, 1), (685, -7, 1)])
def test_edges(stft, L, keyshift, speed, record_margin):
    """constant mode, one frame, the two lengths around the reflect / constant switch (768 | 769 at keyshift 0, 684 | 685 at -7), lengths off
    the hop grid, three frame tiles with a partial last one, a doubled hop: the restatement's frame count and its values"""
    clip = SN.make_clip(L, "mix", seed=11)
    got = stft.get_mel(dev(clip)[None], keyshift=keyshift, speed=speed)[0].cpu().numpy()
    ref = ref64(clip, keyshift, speed)
    assert got.shape == ref.shape == (128, SN.frames(L, keyshift, speed)) and np.isfinite(got).all()
    live = ref != np.log(np.float64(np.float32(SN.CLIP)))
    assert ref[live].min() > np.log(10 * SN.CLIP)
    record_margin(float(np.abs(got.astype(np.float64) - ref).max()), TAIL_TOL)


def _alone(stft, clips, keyshift=0):
    return [stft.get_mel(dev(c)[None], keyshift=keyshift)[0] for c in clips]


@pytest.mark.parametrize("lens", [(3209, 1500, 700), (512 * 40 + 137, 3209, 700, 512 * 17)])
def test_ragged_equals_every_clip_alone(stft, lens):
    """rows [0, F_b) are the clip run alone bit for bit -- its own padding mode and frame count -- whatever the buffer holds beyond the clip
    and whatever a caller's workspace holds; rows beyond are zeros"""
    from lds import native
    clips = [SN.make_clip(n, "mix", seed=20 + b) for b, n in enumerate(lens)]
    alone = _alone(stft, clips)
    Lmax = max(lens)
    n_fft_new, win_new, hop_new, basis, melT = stft._operands(0, 1, torch.device("cuda", torch.cuda.current_device()))
    for fill in (0.0, float("nan"), 1e30):
        buf = np.full((len(lens), Lmax), fill, dtype=np.float32)
        for b, c in enumerate(clips):
            buf[b, :len(c)] = c
        mel, counts = stft.get_mel_ragged(dev(buf), list(lens))
        assert counts == [SN.frames(n) for n in lens] and tuple(mel.shape) == (len(lens), 128, max(counts))
        for b, F in enumerate(counts):
            assert torch.equal(mel[b, :, :F], alone[b]), (fill, b)
            assert not mel[b, :, F:].any()
        for pattern in (0xFF, 0x7F):
            ws = torch.full((1 << 16,), pattern, dtype=torch.uint8, device="cuda")
            out = native.stft_mel(dev(buf), basis, melT, n_fft_new, win_new, hop_new, SN.N_FFT, SN.WIN, SN.CLIP, max(counts), lengths=list(lens), ws=ws)
            assert torch.equal(out.transpose(1, 2), mel), (fill, pattern)


def test_repeatable(stft, fx):
    x = dev(np.stack([fx["clip_0"], fx["clip_4"]]))
    first = stft.get_mel(x, keyshift=5)
    for _ in range(4):
        assert torch.equal(stft.get_mel(x, keyshift=5), first)


def test_round_trip_frame_count():
    """a vocoded latent of T frames has T mel frames (L = 512 T at keyshift 0), reached as the validation pass does: vocoder.vocoder.get_mel"""
    from diffusion.vocoder import Vocoder
    from encoder.hifi_vaegan.hifi_vaegan import Hifi_VAEGAN
    from lds import arch, init_weights
    h = arch.SYNTHETIC_VOCODER_H
    voc = Vocoder.__new__(Vocoder)
    voc.vocoder = Hifi_VAEGAN(None, device="cuda", h=h, state=init_weights.init_state(arch.generator_param_shapes(h), 0))
    T = 37
    z = dev(init_weights.uniform("mel.roundtrip.z", (1, T, h["inter_channels"]), 3, -1.0, 1.0))
    wav = voc.infer(z)
    mel = voc.vocoder.get_mel(wav[0, ...])
    assert tuple(mel.shape) == (1, T, 128) and bool(torch.isfinite(mel).all())
