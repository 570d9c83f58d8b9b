"""`STFT` with the reference's constructor and `get_mel` (reference encoder/hifi_vaegan/modules/nvSTFT.py:55-118): the log-mel spectrogram
the validation pass takes of the vocoder's output.  The whole chain -- padding, framed DFT, magnitude, keyshift cut and scale, mel product,
log -- is one HIP launch (csrc/stftmel.hip); this class resolves the geometry of a (keyshift, speed) pair and keeps the DFT basis and the
filter bank on the device.  `get_mel_ragged` (not in the reference) takes a padded batch of clips of their own lengths.
Reading audio files is not part of this build: `__call__` and `load_wav_to_torch` raise."""
import numpy as np
import torch

from lds import native, stftmel


def load_wav_to_torch(full_path, target_sr=None, return_empty_on_exception=False):
    raise NotImplementedError("load_wav_to_torch reads audio files (soundfile / librosa), which is not part of this build; "
                              "load the waveform yourself and call STFT.get_mel")


class STFT:
    def __init__(self, sr=22050, n_mels=80, n_fft=1024, win_size=1024, hop_length=256, fmin=20, fmax=11025, clip_val=1e-5):
        self.target_sr = sr
        self.n_mels = n_mels
        self.n_fft = n_fft
        self.win_size = win_size
        self.hop_length = hop_length
        self.fmin = fmin
        self.fmax = fmax
        self.clip_val = clip_val
        self.mel_basis = {}       # str(fmax)_device -> the transposed filter bank [n_fft // 2 + 1, n_mels] (the kernel reads it bin-major)
        self.hann_window = {}     # keyshift_device -> the float64 DFT basis with the fp32 window folded in

    def _operands(self, keyshift, speed, device):
        n_fft_new, win_new, hop_new = stftmel.geometry(self.n_fft, self.win_size, self.hop_length, keyshift, speed)
        mel_key = str(self.fmax) + "_" + str(device)
        if mel_key not in self.mel_basis:
            mel = stftmel.slaney_mel(self.target_sr, self.n_fft, self.n_mels, self.fmin, self.fmax)
            self.mel_basis[mel_key] = torch.from_numpy(np.ascontiguousarray(mel.T)).to(device)
        key = str(keyshift) + "_" + str(device)
        if key not in self.hann_window:
            bins = min(n_fft_new // 2 + 1, self.n_fft // 2 + 1)
            window = torch.hann_window(win_new).numpy()      # the reference's fp32 window values
            self.hann_window[key] = torch.from_numpy(stftmel.dft_basis(n_fft_new, bins, window)).to(device)
        return n_fft_new, win_new, hop_new, self.hann_window[key], self.mel_basis[mel_key]

    def _run(self, y, lengths, keyshift, speed, center):
        if center:
            raise NotImplementedError("STFT.get_mel: center=True is not built (nothing in the reference passes it)")
        if not y.is_cuda:
            raise RuntimeError("STFT.get_mel needs tensors on a HIP device (no CPU fallback)")
        if y.dim() == 1:
            y = y[None]
        y = y.float().contiguous()
        n_fft_new, win_new, hop_new, basis, melT = self._operands(keyshift, speed, y.device)
        L = y.shape[-1]
        counts = [stftmel.frames(int(n), n_fft_new, win_new, hop_new) for n in (lengths if lengths is not None else [L])]
        if min(counts) < 1:
            raise ValueError(f"STFT.get_mel: a clip is shorter than one transform of {n_fft_new} samples after padding")
        out = native.stft_mel(y, basis, melT, n_fft_new, win_new, hop_new, self.n_fft, self.win_size, float(self.clip_val), max(counts), lengths=lengths)
        return out, counts

    def get_mel_frames(self, y, keyshift=0, speed=1, center=False):
        """get_mel as the kernel stores it: [B, F, n_mels] (what Hifi_VAEGAN.get_mel returns; no transpose in between)"""
        return self._run(y, None, keyshift, speed, center)[0]

    def get_mel(self, y, keyshift=0, speed=1, center=False):
        """y [B, L] (or [L]) on the device -> log-mel [B, n_mels, F]"""
        return native.transpose(self.get_mel_frames(y, keyshift, speed, center))

    def get_mel_ragged(self, y, lengths, keyshift=0):
        """Extension (not in the reference): y [B, L] padded to the longest clip + every clip's own sample count (host ints, B <= 64) ->
        (log-mel [B, n_mels, F], frame counts [B]) with every clip analysed as if alone -- its own padding mode and frame count, whatever
        the buffer holds beyond lengths[b]; columns at and beyond a clip's frames are zeros."""
        ln = native._host_lengths(lengths, y.shape[0], 1, y.shape[-1], 64, "log-mel")
        out, counts = self._run(y, ln, keyshift, 1, False)
        return native.transpose(out), counts

    def __call__(self, audiopath):
        raise NotImplementedError("STFT.__call__ reads an audio file, which is not part of this build; call get_mel on a waveform tensor")


stft = STFT()
