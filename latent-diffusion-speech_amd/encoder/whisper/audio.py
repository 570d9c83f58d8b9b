"""Whisper's audio front end on the native kernels (reference encoder/whisper/audio.py:9-82): the constants, `mel_filters` and
`log_mel_spectrogram`.  `load_audio` (an ffmpeg subprocess) and `pad_or_trim` are not on the units path and are not built."""
from functools import lru_cache

import numpy as np
import torch

from lds import arch, native

SAMPLE_RATE = 16000
N_FFT = 400
HOP_LENGTH = 160
CHUNK_LENGTH = 30
N_SAMPLES = CHUNK_LENGTH * SAMPLE_RATE  # 480000 samples in a 30-second chunk


@lru_cache(maxsize=None)
def mel_filters(device, n_mels: int) -> torch.Tensor:
    """[n_mels, 201] float32.  The reference loads assets/mel_filters.npz; here the same bank is computed (lds.arch.whisper_mel_filters:
    librosa's Slaney-scale formula in float64, rounded once; within 4e-9 of the reference's file)."""
    assert n_mels in {80, 128}, f"Unsupported n_mels: {n_mels}"
    return torch.from_numpy(arch.whisper_mel_filters(n_mels)).to(device)


@lru_cache(maxsize=None)
def _front_end(n_mels):
    """a handle used for its front end only: the smallest encoder the library accepts, zero weights"""
    shapes = arch.whisper_param_shapes(n_mels, 64, 1)
    return native.Whisper(n_mels, 64, 1, 1, 1 << 16, {k: np.zeros(s, dtype=np.float32) for k, s in shapes.items()}, arch.whisper_mel_filters(n_mels))


def log_mel_spectrogram(audio, n_mels: int = 128, padding: int = 0, device=None):
    """audio [L] or [B, L] (tensor or numpy, 16 kHz) -> [n_mels, L // 160] or [B, n_mels, L // 160] on the device.
    Deviations from the reference: the result needs a HIP device (`device`, or the tensor's own; CPU tensors raise, there is no CPU
    fallback); a file name is not accepted (load_audio is not built); the dynamic-range floor `max - 8` is taken per clip, where the
    reference takes one maximum over the whole batch -- the units path only ever passes one clip (tools/tools.py:120)."""
    if isinstance(audio, str):
        raise NotImplementedError("log_mel_spectrogram: loading a file needs ffmpeg (load_audio), which is not built; pass samples")
    if not torch.is_tensor(audio):
        audio = torch.from_numpy(np.asarray(audio))
    if device is not None:
        audio = audio.to(device)
    if not audio.is_cuda:
        raise RuntimeError("log_mel_spectrogram needs the audio on a HIP device (no CPU fallback)")
    if padding > 0:
        audio = torch.nn.functional.pad(audio, (0, padding))
    a = audio.float().reshape(-1, audio.shape[-1]).contiguous()
    mel = _front_end(n_mels).logmel(a)
    return mel.reshape(tuple(audio.shape[:-1]) + mel.shape[1:])
