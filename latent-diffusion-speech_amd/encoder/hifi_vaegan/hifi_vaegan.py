"""`Hifi_VAEGAN` wrapper (reference encoder/hifi_vaegan/hifi_vaegan.py:10-65): reads
`<model_path>/decoder.pth` = {'config': h, 'model': state_dict with weight-norm pairs}, lazily
builds the native Generator on first call and maps z [B,T,C] -> wav [B,1,T*hop]; `extract` lazily
builds the native encoder from `<model_path>/encoder.pth` (same layout) and maps audio [B,L] -> [B,T,2C]; `extract_ragged` does the same
for a batch of clips of their own lengths; `get_mel` is the log-mel analysis of a waveform (csrc/stftmel.hip)."""
import os

import torch

from lds import native

from .modules.nvSTFT import STFT


def load_config(model_path):
    h = torch.load(os.path.join(model_path, "decoder.pth"), map_location="cpu", weights_only=False)["config"]
    return h


class Hifi_VAEGAN(torch.nn.Module):
    def __init__(self, model_path, device=None, h=None, state=None, *, encoder_state=None):
        """`h`/`state` (optional, not in the reference) inject a config + Generator state_dict directly,
        for synthetic-weight runs where no decoder.pth exists; `encoder_state` likewise an Encoder state_dict
        (no encoder.pth)."""
        super().__init__()
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.device = device
        self.model_path = model_path
        self.encoder_model = None
        self.decoder_model = None
        self._state = state
        self._encoder_state = encoder_state
        self.h = h if h is not None else load_config(model_path)
        self.stft = STFT(self.h["sampling_rate"], 128, 2048, 2048, 512, 40, 16000)

    def sample_rate(self):
        return self.h["sampling_rate"]

    def hop_size(self):
        return self.h["hop_size"]

    def dimension(self):
        return self.h["inter_channels"]

    @torch.no_grad()
    def get_mel(self, audio, keyshift=0):
        """audio [B,L] -> the log-mel spectrogram [B,F,128] the validation pass compares (reference hifi_vaegan.py:67-70); stored
        frame-major by the kernel, so no transpose runs"""
        return self.stft.get_mel_frames(audio, keyshift=keyshift)

    @torch.no_grad()
    def extract(self, audio, only_z=False, only_mean=False, *, noise=None):
        """audio [B,L] -> cat(m, logs) as [B,T,2C] (logs zeroed under only_mean), or z = m + randn * exp(logs) as [B,T,C] under only_z
        (reference hifi_vaegan.py:32-50).  L is right-padded with zeros to a multiple of the hop.  The reference draws randn_like(m)
        inside every encoder call; so does this one (torch.randn of [B,C,T] on the device), so the torch generator advances the same.
        `noise` (not in the reference): a [B,C,T] tensor used instead of that draw (nothing is drawn then)."""
        if not audio.is_cuda:
            raise RuntimeError("Hifi_VAEGAN.extract needs tensors on a HIP device (no CPU fallback)")
        return self._encode(audio, only_z, only_mean, noise, None)

    @torch.no_grad()
    def extract_ragged(self, audio, lengths, only_z=False, only_mean=False, *, noise=None):
        """Extension (not in the reference): audio [B,L] padded to the longest clip + every clip's own sample count (host ints, B <= 64,
        1 .. L) -> [B,T,2C] (or z [B,T,C] under only_z) with every clip encoded as if alone: clip b is audio[b, :lengths[b]] right-padded
        with zeros to T_b = ceil(lengths[b] / hop) frames, whatever the buffer holds beyond lengths[b]; rows [T_b, T) are zeros
        (include/lds.h lds_vae_encoder_forward_ragged).  Pads L and draws the noise exactly as extract does; z uses noise[b, :, :T_b]."""
        B, L = audio.shape[0], audio.shape[-1]
        ln = native.VaeEncoder.lengths(lengths, B, L)      # (host-side validation first: a bad length is a ValueError on any device)
        if not audio.is_cuda:
            raise RuntimeError("Hifi_VAEGAN.extract_ragged needs tensors on a HIP device (no CPU fallback)")
        return self._encode(audio, only_z, only_mean, noise, ln)

    def _encode(self, audio, only_z, only_mean, noise, lengths):
        if self.encoder_model is None:
            state = self._encoder_state
            if state is None:
                print("| Load Vaegan Encoder: ", self.model_path)
                state = torch.load(os.path.join(self.model_path, "encoder.pth"), map_location="cpu", weights_only=False)["model"]
            self.encoder_model = native.VaeEncoder(self.h, state)     # folds weight norm like remove_weight_norm()
            self._encoder_state = None
        audio = audio.float()
        hop = self.hop_size()
        if audio.shape[-1] % hop != 0:      # PAD
            audio = torch.nn.functional.pad(audio, (0, hop - audio.shape[-1] % hop))
        audio = audio.contiguous()
        B, T = audio.shape[0], audio.shape[-1] // hop
        if noise is None:
            noise = torch.randn(B, self.dimension(), T, dtype=torch.float32, device=audio.device)      # randn_like(m)
        out, z = self.encoder_model.forward(audio, noise.float().contiguous() if only_z else None, only_mean=only_mean, lengths=lengths)
        return z if only_z else out

    @torch.no_grad()
    def forward_ragged(self, z, lengths):
        """Extension (not in the reference): z [B,T,C] padded to the longest utterance + per-utterance frame counts -> wav [B,1,T*hop] with
        zeros beyond each utterance's samples; every utterance as if it were decoded alone (include/lds.h lds_vocoder_forward_ragged)"""
        return self._decode(z, lengths)

    @torch.no_grad()
    def forward(self, z):
        return self._decode(z, None)

    def _decode(self, z, _lengths):
        if not z.is_cuda:
            raise RuntimeError("Hifi_VAEGAN.forward needs tensors on a HIP device (no CPU fallback)")
        if self.decoder_model is None:
            state = self._state
            if state is None:
                print("| Load Vaegan:", self.model_path)
                state = torch.load(os.path.join(self.model_path, "decoder.pth"), map_location="cpu", weights_only=False)["model"]
            self.decoder_model = native.Generator(self.h, state)     # folds weight norm like remove_weight_norm()
            self._state = None
        zt = native.transpose(z.contiguous().float())                # z.transpose(-1,-2) -> [B,C,T]
        return self.decoder_model.forward(zt, _lengths)
