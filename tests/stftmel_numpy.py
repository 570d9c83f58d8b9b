"""float64 restatements of the vocoder's log-mel analysis (reference encoder/hifi_vaegan/modules/nvSTFT.py:69-118, STFT.get_mel with
center = False) and of librosa.filters.mel's defaults: what tests/test_cpu_mel.py and tests/test_gpu_mel.py compare against, and what
tests/golden/make_mel_fixtures.py evaluates beside the reference's own fp32 run.  numpy only."""
import numpy as np

# STFT(sr, 128, 2048, 2048, 512, 40, 16000): the instance Hifi_VAEGAN builds
SR, N_MELS, N_FFT, WIN, HOP, FMIN, FMAX, CLIP = 44100, 128, 2048, 2048, 512, 40, 16000, 1e-5
LENGTHS = (3072, 3209, 1500, 700)
KEYSHIFTS = (0, 5, -7, 12, -12)


def geometry(keyshift=0, speed=1, n_fft=N_FFT, win=WIN, hop=HOP):
    factor = 2 ** (keyshift / 12)
    return int(np.round(n_fft * factor)), int(np.round(win * factor)), int(np.round(hop * speed))


def padding(L, win_new, hop_new):
    pad_left = (win_new - hop_new) // 2
    pad_right = max((win_new - hop_new + 1) // 2, win_new - L - pad_left)
    return pad_left, pad_right, "reflect" if pad_right < L else "constant"


def frames(L, keyshift=0, speed=1, n_fft=N_FFT, win=WIN, hop=HOP):
    n_fft_new, win_new, hop_new = geometry(keyshift, speed, n_fft, win, hop)
    pad_left, pad_right, _ = padding(L, win_new, hop_new)
    return 1 + (L + pad_left + pad_right - n_fft_new) // hop_new


def hann64(n):
    """torch.hann_window(n) (periodic) in float64"""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n, dtype=np.float64) / n)


def slaney_mel64(sr=SR, n_fft=N_FFT, n_mels=N_MELS, fmin=FMIN, fmax=FMAX):
    """librosa.filters.mel(htk=False, norm='slaney') in float64 [n_mels, n_fft // 2 + 1]"""
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0

    def to_mel(f):
        return min_log_mel + np.log(f / min_log_hz) / logstep if f >= min_log_hz else f / f_sp

    pts = np.linspace(to_mel(float(fmin)), to_mel(float(fmax)), n_mels + 2)
    hz = np.where(pts >= min_log_mel, min_log_hz * np.exp(logstep * (pts - min_log_mel)), f_sp * pts)
    freqs = np.arange(n_fft // 2 + 1, dtype=np.float64) * (float(sr) / n_fft)
    w = np.zeros((n_mels, len(freqs)))
    for i in range(n_mels):
        lower = (freqs - hz[i]) / (hz[i + 1] - hz[i])
        upper = (hz[i + 2] - freqs) / (hz[i + 2] - hz[i + 1])
        w[i] = np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (hz[i + 2] - hz[i]))
    return w


def get_mel64(y, window, bank, keyshift=0, speed=1, n_fft=N_FFT, win=WIN, hop=HOP, clip_val=np.float32(CLIP)):
    """the reference's lines in float64 on one clip y [L]; `window` [win_new] and `bank` [n_mels, n_fft // 2 + 1] are data (the fp32 values
    the reference holds, or float64 ones) -> log-mel float64 [n_mels, F]"""
    y = np.asarray(y, dtype=np.float64)
    n_fft_new, win_new, hop_new = geometry(keyshift, speed, n_fft, win, hop)
    pad_left, pad_right, mode = padding(len(y), win_new, hop_new)
    yp = np.pad(y, (pad_left, pad_right), mode=mode)
    F = 1 + (len(yp) - n_fft_new) // hop_new
    w = np.zeros(n_fft_new)
    left = (n_fft_new - win_new) // 2
    w[left:left + win_new] = np.asarray(window, dtype=np.float64)
    fr = np.stack([yp[f * hop_new:f * hop_new + n_fft_new] for f in range(F)]) * w[None, :]
    spec = np.fft.rfft(fr, axis=1).T                                  # [n_fft_new // 2 + 1, F]
    mag = np.sqrt(spec.real ** 2 + spec.imag ** 2 + 1e-9)
    if keyshift != 0:
        size = n_fft // 2 + 1
        if mag.shape[0] < size:
            mag = np.concatenate([mag, np.zeros((size - mag.shape[0], F))])
        mag = mag[:size] * win / win_new
    mel = np.asarray(bank, dtype=np.float64) @ mag
    return np.log(np.maximum(mel, np.float64(clip_val)))


def make_clip(L, kind="mix", seed=0):
    """fp32 [L]: 'mix' = a 440 Hz sine + a 200 Hz .. 20 kHz chirp + 0.05-rms noise; 'noise' = 0.2-rms noise.  Every mel band of either sits
    at least 10 x above clip_val (the band that straddles a negative keyshift's cut keeps a sliver of its triangle and is the smallest, 5.7e-4),
    so the log is never taken near the clamp."""
    rng = np.random.RandomState(1234 + seed)
    n = np.arange(L, dtype=np.float64)
    noise = rng.standard_normal(L)
    if kind == "noise":
        return (0.2 * noise).astype(np.float32)
    t = n / SR
    dur = L / SR
    chirp = np.sin(2 * np.pi * (200.0 * t + 0.5 * (20000.0 - 200.0) / dur * t * t))
    return (0.3 * np.sin(2 * np.pi * 440.0 * t) + 0.3 * chirp + 0.05 * noise).astype(np.float32)


CLIPS = [("mix", L) for L in LENGTHS] + [("noise", 3072)]
