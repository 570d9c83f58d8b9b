"""Host side of the vocoder's log-mel analysis (csrc/stftmel.hip; reference encoder/hifi_vaegan/modules/nvSTFT.py:69-118): the geometry
of a (keyshift, speed) pair, the float64 windowed DFT basis, and the Slaney mel filter bank the reference takes from librosa."""
import numpy as np


def geometry(n_fft, win_size, hop_length, keyshift=0, speed=1):
    """(n_fft_new, win_new, hop_new) of nvSTFT.py:79-82 (Python's round-half-even on the float64 products, as np.round gives)"""
    factor = 2 ** (keyshift / 12)
    return int(np.round(n_fft * factor)), int(np.round(win_size * factor)), int(np.round(hop_length * speed))


def padding(L, win_new, hop_new):
    """(pad_left, pad_right, mode) of a clip of L samples (nvSTFT.py:98-103)"""
    pad_left = (win_new - hop_new) // 2
    pad_right = max((win_new - hop_new + 1) // 2, win_new - L - pad_left)
    return pad_left, pad_right, "reflect" if pad_right < L else "constant"


def frames(L, n_fft_new, win_new, hop_new):
    """frames torch.stft(center=False) takes from the padded clip (0 when it is shorter than one transform)"""
    pad_left, pad_right, _ = padding(L, win_new, hop_new)
    total = L + pad_left + pad_right - n_fft_new
    return 0 if total < 0 else 1 + total // hop_new


def dft_basis(n_fft_new, bins, window):
    """float64 [n_fft_new][bins][2]: (cos, -sin)(2 pi n k / n_fft_new) times window[n]; `window` (the reference's fp32 torch.hann_window(win_new)
    values) is centred in n_fft_new as torch.stft does.  The angle is reduced in integers: (n k) mod n_fft_new is exact, so every entry is
    the float64 rounding of the true value however large n k gets."""
    w = np.zeros(n_fft_new, dtype=np.float64)
    left = (n_fft_new - len(window)) // 2
    w[left:left + len(window)] = np.asarray(window, dtype=np.float64)
    r = (np.arange(n_fft_new, dtype=np.int64)[:, None] * np.arange(bins, dtype=np.int64)[None, :]) % n_fft_new
    ang = r.astype(np.float64) * (2.0 * np.pi / n_fft_new)
    out = np.empty((n_fft_new, bins, 2), dtype=np.float64)
    out[:, :, 0] = np.cos(ang) * w[:, None]
    out[:, :, 1] = -np.sin(ang) * w[:, None]
    return out


def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, min_log_hz) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def slaney_mel(sr, n_fft, n_mels, fmin, fmax):
    """librosa.filters.mel(sr=, n_fft=, n_mels=, fmin=, fmax=) with its defaults (Slaney scale, Slaney area normalisation): triangles between
    n_mels + 2 points equally spaced on the mel scale, evaluated in float64 and rounded once to fp32 [n_mels, n_fft // 2 + 1]."""
    if fmax is None:
        fmax = sr / 2.0
    fftfreqs = np.arange(n_fft // 2 + 1, dtype=np.float64) * (float(sr) / n_fft)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fftfreqs[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    weights = np.maximum(0.0, np.minimum(lower, upper))
    weights *= (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]
    return weights.astype(np.float32)
