"""Host side of the validation pass (no GPU): the float64 restatement of the reference's STFT.get_mel (tests/stftmel_numpy.py) against what
the reference recorded (tests/golden/vocoder_mel.npz, made by tests/golden/make_mel_fixtures.py), the geometry of a (keyshift, speed) pair
around the reflect / constant switch, the Slaney filter bank and the DFT basis of lds/stftmel.py, and the errors raised before any device
call."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

import stftmel_numpy as SN
from conftest import GOLDEN


def _window(win_new):
    import torch
    return torch.hann_window(win_new).numpy()


def test_restatement_reproduces_the_recorded_reference(golden):
    """ref64 of the fixture is get_mel64 with the reference's fp32 window and bank as data; the recorded reference error is the fp32 scale"""
    g = golden("vocoder_mel.npz")
    for i, (kind, L) in enumerate(SN.CLIPS):
        assert np.array_equal(g[f"clip_{i}"], SN.make_clip(L, kind, seed=i))
        for k in SN.KEYSHIFTS:
            ref = g[f"ref64_{i}_{k}"]
            got = SN.get_mel64(g[f"clip_{i}"], _window(SN.geometry(k)[1]), g["bank"], keyshift=k)
            assert got.shape == ref.shape == (SN.N_MELS, SN.frames(L, k))
            assert np.abs(got - ref).max() < 1e-9, (i, k)
            assert 1e-8 < float(g[f"eref_{i}_{k}"]) < 5e-5, (i, k)
    # a negative keyshift zeroes the bins beyond its own Nyquist: the mel rows that see only those sit exactly on the clamp
    floor = np.log(np.float64(np.float32(SN.CLIP)))
    assert (g["ref64_0_-12"][-1] == floor).all() and not (g["ref64_0_0"] == floor).any()


def test_geometry_and_the_mode_switch():
    from lds import stftmel
    for k in SN.KEYSHIFTS + (0.001,):
        for speed in (1, 2, 0.5):
            assert stftmel.geometry(SN.N_FFT, SN.WIN, SN.HOP, k, speed) == SN.geometry(k, speed)
    assert [SN.geometry(k)[0] for k in (-12, -7, 5, 12)] == [1024, 1367, 2734, 4096]
    # keyshift 0: pad_left 768, pad_right max(768, 1280 - L); reflect needs pad_right < L: the switch sits between 768 and 769 samples
    table = {700: (768, 768, "constant", 1), 767: (768, 768, "constant", 1), 768: (768, 768, "constant", 1), 769: (768, 768, "reflect", 1),
             511: (768, 769, "constant", 1), 1: (768, 1279, "constant", 1), 1500: (768, 768, "reflect", 2), 2048 - 768: (768, 768, "reflect", 2),
             3072: (768, 768, "reflect", 6), 3209: (768, 768, "reflect", 6), 512 * 9 + 137: (768, 768, "reflect", 9)}
    for L, (pl, pr, mode, F) in table.items():
        assert stftmel.padding(L, 2048, 512) == SN.padding(L, 2048, 512) == (pl, pr, mode), L
        assert stftmel.frames(L, 2048, 2048, 512) == SN.frames(L) == F, L
    for T in (1, 2, 37, 512):      # a vocoded latent of T frames has T mel frames
        assert stftmel.frames(512 * T, 2048, 2048, 512) == T
    # the switch under a keyshift and a speed: constant while pad_right >= L, reflect from the first L with pad_right < L
    for k, speed in ((-7, 1), (5, 1), (12, 1), (0, 2)):
        n_fft_new, win_new, hop_new = SN.geometry(k, speed)
        first = next(L for L in range(1, win_new) if SN.padding(L, win_new, hop_new)[2] == "reflect")
        pl, pr, mode = stftmel.padding(first - 1, win_new, hop_new)
        assert mode == "constant" and pr >= first - 1
        pl, pr, mode = stftmel.padding(first, win_new, hop_new)
        assert mode == "reflect" and pl <= pr < first
        for L in (first - 1, first, first + 1, 3209):
            assert stftmel.padding(L, win_new, hop_new) == SN.padding(L, win_new, hop_new)
            assert stftmel.frames(L, n_fft_new, win_new, hop_new) == SN.frames(L, k, speed) >= 1


def test_filter_bank(golden):
    from lds import stftmel
    bank = stftmel.slaney_mel(SN.SR, SN.N_FFT, SN.N_MELS, SN.FMIN, SN.FMAX)
    ref = SN.slaney_mel64()
    assert bank.dtype == np.float32 and bank.shape == (128, 1025)
    assert np.abs(bank.astype(np.float64) - ref).max() <= 2.0 ** -23 * ref.max()       # two spellings of the formula, one fp32 rounding
    assert np.abs(bank.astype(np.float64) - golden("vocoder_mel.npz")["bank"]).max() <= 2.0 ** -23 * ref.max()
    assert (bank >= 0).all() and (bank.max(axis=1) > 0).all()                           # no empty band at 128 / 2048 / 40 .. 16000
    nz = (bank > 0).sum(axis=1)
    assert nz.min() >= 1 and nz.max() <= 64
    # Slaney normalisation: every triangle has unit area in Hz; the sampled sum is that within the bin spacing over the band's width
    df = SN.SR / SN.N_FFT
    area = ref.sum(axis=1) * df
    assert abs(area[-1] - 1) < 0.02 and (np.abs(area - 1) < 0.5).all(), (area.min(), area.max())
    peaks = bank.argmax(axis=1)
    assert (np.diff(peaks) >= 0).all() and peaks[0] >= 1 and peaks[-1] <= int(SN.FMAX / df) + 1
    assert not bank[:, int(SN.FMAX / df) + 2:].any()
    assert stftmel.slaney_mel(22050, 1024, 80, 20, None).shape == (80, 513)


@pytest.mark.parametrize("n", [64, 70, 1367])
def test_dft_basis_is_the_windowed_rfft(n):
    from lds import stftmel
    win = n - 6 if n == 70 else n
    w = _window(win)
    basis = stftmel.dft_basis(n, n // 2 + 1, w)
    assert basis.shape == (n, n // 2 + 1, 2) and basis.dtype == np.float64
    x = np.random.RandomState(3).standard_normal((3, n))
    wp = np.zeros(n)
    wp[(n - win) // 2:(n - win) // 2 + win] = w
    ref = np.fft.rfft(x * wp, axis=1)
    got = x @ basis[:, :, 0] + 1j * (x @ basis[:, :, 1])
    assert np.abs(got - ref).max() < 1e-11 * n
    # the angle is reduced in integers: entries whose n k agree modulo n are the same bits, however large n k is
    one = stftmel.dft_basis(n, n // 2 + 1, np.ones(n))
    assert np.array_equal(one[n - 1, 2], one[n - 2, 1]) and np.array_equal(one[6, 1], one[2, 3]) and np.array_equal(one[n - 3, n // 2], one[n - n // 2, 3])


def test_api_and_errors_before_any_device_call():
    import torch
    from diffusion.diffusion import GaussianDiffusion
    from diffusion.unit2mel import Unit2Mel
    from encoder.hifi_vaegan.hifi_vaegan import Hifi_VAEGAN
    from encoder.hifi_vaegan.modules import nvSTFT
    from lds import arch
    sig = inspect.signature(nvSTFT.STFT.__init__)
    assert list(sig.parameters)[1:] == ["sr", "n_mels", "n_fft", "win_size", "hop_length", "fmin", "fmax", "clip_val"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == [22050, 80, 1024, 1024, 256, 20, 11025, 1e-5]
    g = inspect.signature(nvSTFT.STFT.get_mel)
    assert list(g.parameters)[1:] == ["y", "keyshift", "speed", "center"] and g.parameters["center"].default is False
    s = nvSTFT.STFT(44100, 128, 2048, 2048, 512, 40, 16000)
    with pytest.raises(NotImplementedError):
        s.get_mel(torch.zeros(1, 4096), center=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.get_mel(torch.zeros(1, 4096))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.get_mel_ragged(torch.zeros(2, 4096), [4096, 700])
    with pytest.raises(ValueError):
        s.get_mel_ragged(torch.zeros(2, 4096), [4096, 5000])
    with pytest.raises(NotImplementedError):
        s("some.wav")
    with pytest.raises(NotImplementedError):
        nvSTFT.load_wav_to_torch("some.wav")
    v = Hifi_VAEGAN(None, device="cpu", h=arch.SYNTHETIC_VOCODER_H, state={})
    assert isinstance(v.stft, nvSTFT.STFT) and (v.stft.n_mels, v.stft.n_fft, v.stft.win_size, v.stft.hop_length, v.stft.fmin, v.stft.fmax) == \
        (128, 2048, 2048, 512, 40, 16000) and v.stft.target_sr == arch.SYNTHETIC_VOCODER_H["sampling_rate"]
    assert list(inspect.signature(Hifi_VAEGAN.get_mel).parameters)[1:] == ["audio", "keyshift"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        v.get_mel(torch.zeros(1, 4096))
    p = inspect.signature(GaussianDiffusion.p_losses)
    assert list(p.parameters)[1:] == ["x_start", "t", "cond", "noise", "loss_type"] and p.parameters["loss_type"].default == "l2"
    gd = GaussianDiffusion(torch.nn.Identity(), out_dims=80)
    with pytest.raises(NotImplementedError):
        gd.p_losses(torch.zeros(1, 1, 80, 8), torch.zeros(1, dtype=torch.long), torch.zeros(1, 256, 8), loss_type="huber")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gd.p_losses(torch.zeros(1, 1, 80, 8), torch.zeros(1, dtype=torch.long), torch.zeros(1, 256, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gd(torch.zeros(1, 8, 256), gt_spec=torch.zeros(1, 8, 80), infer=False)
    for fn in (GaussianDiffusion.loss, Unit2Mel.loss):
        kw = [n for n, q in inspect.signature(fn).parameters.items() if q.kind is inspect.Parameter.KEYWORD_ONLY]
        assert kw == ["t", "noise", "loss_type"]


def test_recipe_regenerates_the_committed_fixtures():
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_mel_fixtures.py"), "--verify"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode == 3:
        pytest.skip("the reference checkout is not on this machine")
    assert r.returncode == 0 and "fixtures reproduce" in r.stdout, r.stdout[-2000:]
