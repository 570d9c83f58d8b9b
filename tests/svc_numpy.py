"""float64 restatements for the long-audio tests (no torch, no library code), in the manner of tests/resample_numpy.py:
  frame_rms           librosa.feature.rms(y=y, frame_length, hop_length, center=True, pad_mode): sqrt of the mean square of every frame of
                      the signal padded by frame_length // 2 on both sides;
  to_mono             librosa.to_mono: the mean over the channel axis;
  volume / mask       Volume_Extractor.extract and get_mask_from_volume + upsample (reference tools/tools.py:23-41, 225-229) by their
                      formulas: frame k = mean of the reflect-padded squares over int(k hop) .. int((k + 1) hop); m = volume > thr, dilated
                      over 4 frames either side, then interpolated linearly at j / factor with the last frame repeated;
  assemble            the sequential loop of DiffusionSVC.infer_from_long_audio (reference tools/infer_tools.py:105-115 with
                      tools/tools.py:231-238): mask product, zero gaps, cross-fade over the overlap."""
import numpy as np


def frame_rms_length(L, frame_length, hop_length):
    return 1 + (int(L) + 2 * (frame_length // 2) - frame_length) // hop_length


def frame_rms(y, frame_length=2048, hop_length=512, center=True, pad_mode="constant"):
    y = np.asarray(y, dtype=np.float64)
    if center:
        y = np.pad(y, frame_length // 2, mode=pad_mode)
    n = 1 + (len(y) - frame_length) // hop_length
    sq = y * y
    return np.sqrt(np.array([sq[t * hop_length: t * hop_length + frame_length].mean() for t in range(n)]))


def to_mono(y):
    y = np.asarray(y)
    return y.mean(axis=0) if y.ndim > 1 else y


def volume(audio, hop):
    audio = np.asarray(audio, dtype=np.float64)
    hop = float(hop)
    n = int(len(audio) // hop) + 1
    sq = np.pad(audio * audio, (int(hop // 2), int((hop + 1) // 2)), mode="reflect")
    return np.sqrt(np.array([sq[int(k * hop): int((k + 1) * hop)].mean() for k in range(n)]))


def mask(vol, threshold, factor):
    """threshold: the linear amplitude (10 ** (dB / 20)); -> [n * factor]"""
    m = (np.asarray(vol) > threshold).astype(np.float64)
    n = len(m)
    M = np.array([m[max(k - 4, 0): min(k + 4, n - 1) + 1].max() for k in range(n)])
    j = np.arange(n * factor)
    i = j // factor
    f = (j % factor) / factor
    return M[i] * (1 - f) + M[np.minimum(i + 1, n - 1)] * f


def assemble(segments, starts, mask_=None):
    """segments: list of 1-D arrays; starts: their first samples in the result; mask_: array at least as long as the result, or None"""
    result = np.zeros(0)
    for seg, start in zip(segments, starts):
        v = np.asarray(seg, dtype=np.float64)
        if mask_ is not None:
            v = v * np.asarray(mask_, dtype=np.float64)[start: start + len(v)]
        if start >= len(result):
            result = np.concatenate([result, np.zeros(start - len(result)), v])
        else:
            F = len(result) - start
            k = np.linspace(0, 1.0, num=F, endpoint=True)
            faded = (1 - k) * result[start:] + k * v[:F]
            result = np.concatenate([result[:start], faded, v[F:]])
    return result


# ---- the fixture clip: a tone under a piecewise-linear envelope (deterministic; every decision of the slicer has a margin) ------------
# (seconds, amplitude) breakpoints: loud stretches at 0.2 .. 0.3, silences that ramp between 6e-4 and 1e-4 with one lowest point each
ENVELOPE = [(0.00, 6e-4), (0.37, 1e-4), (0.60, 5e-4), (0.65, 0.25), (1.50, 0.30), (1.55, 6e-4), (1.83, 1e-4), (2.00, 4e-4), (2.05, 0.20),
            (3.20, 0.30), (3.25, 6e-4), (3.52, 1e-4), (4.10, 6e-4), (4.15, 0.25), (4.90, 0.20), (4.95, 5e-4), (5.23, 1e-4), (5.35, 3e-4)]
CLIP_SECONDS, CLIP_TONE = 5.35, 250.0


def make_clip(sr=16000, dtype=np.float32):
    """the 5.35 s fixture clip at `sr` (85,600 samples at 16 kHz)"""
    t = np.arange(int(round(CLIP_SECONDS * sr))) / float(sr)
    env = np.interp(t, [p[0] for p in ENVELOPE], [p[1] for p in ENVELOPE])
    return (env * np.sin(2 * np.pi * CLIP_TONE * t)).astype(dtype)
