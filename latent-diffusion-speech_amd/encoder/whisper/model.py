"""Whisper's audio encoder as parameter holders over the native handle (reference encoder/whisper/model.py:10-137).  The modules carry
the reference's `state_dict` keys, so a reference checkpoint's `model_state_dict` loads unchanged; `AudioEncoder.forward(mel)` runs
lds_whisper_encode_mel.  The reference's `Whisper(dims)` builds no decoder, and neither does this one."""
from dataclasses import dataclass

import torch
from torch import nn

from lds import arch, native


@dataclass
class ModelDimensions:
    n_mels: int
    n_audio_ctx: int
    n_audio_state: int
    n_audio_head: int
    n_audio_layer: int
    n_vocab: int
    n_text_ctx: int
    n_text_state: int
    n_text_head: int
    n_text_layer: int


class AudioEncoder(nn.Module):
    def __init__(self, n_mels: int, n_state: int, n_head: int, n_layer: int, n_ctx: int = 1500):
        """`n_ctx` (not in the reference, whose table is built for whatever length arrives): rows of the sinusoid table = the longest
        input in frames."""
        super().__init__()
        for k, s in arch.whisper_param_shapes(n_mels, n_state, n_layer).items():
            self._register(k[len("encoder."):], torch.zeros(s))
        self.n_mels, self.n_audio_state, self.n_head, self.n_layer, self.n_ctx = n_mels, n_state, n_head, n_layer, n_ctx
        self._native = None

    def _register(self, name, value):
        mod = self
        parts = name.split(".")
        for p in parts[:-1]:
            if not hasattr(mod, p):
                mod.add_module(p, nn.Module())
            mod = getattr(mod, p)
        mod.register_parameter(parts[-1], nn.Parameter(value, requires_grad=False))

    def _load_from_state_dict(self, *a, **k):
        self._native = None      # (new weights: the packed copy is rebuilt on the next call)
        return super()._load_from_state_dict(*a, **k)

    def native(self):
        if self._native is None:
            state = {"encoder." + k: v.detach().cpu() for k, v in self.state_dict().items()}
            self._native = native.Whisper(self.n_mels, self.n_audio_state, self.n_head, self.n_layer, self.n_ctx, state,
                                          arch.whisper_mel_filters(self.n_mels))
        return self._native

    @torch.no_grad()
    def forward(self, x, n_frames=None):
        """mel [B, n_mels, F] on a HIP device -> [B, (F - 1) // 2 + 1, n_state]; n_frames (extension): every clip's own mel frames"""
        if not x.is_cuda:
            raise RuntimeError("AudioEncoder.forward needs the mel on a HIP device (no CPU fallback)")
        return self.native().encode_mel(x.float().contiguous(), n_frames)


class Whisper(nn.Module):
    def __init__(self, dims: ModelDimensions):
        super().__init__()
        self.dims = dims
        self.encoder = AudioEncoder(dims.n_mels, dims.n_audio_state, dims.n_audio_head, dims.n_audio_layer, dims.n_audio_ctx)

    def load_state_dict(self, state_dict, *a, **k):
        self.encoder._native = None
        return super().load_state_dict(state_dict, *a, **k)

    def embed_audio(self, mel):
        return self.encoder(mel)

    @property
    def device(self):
        return next(self.parameters()).device
