"""WavLM as a parameter holder over the native handle: transformers' WavLMModel (so-vits-svc's `wavlmbase+`, kNN-VC's WavLM-Large) in its
two flavours, lds.arch.wavlm_dims("base+" | "large").  The module carries the tensors inference reads under the keys of
WavLMModel.state_dict() (lds.arch.wavlm_param_shapes); `forward` runs lds_wavlm_encode.  The masking, the training path and the task heads
(CTC, x-vector, ...) are not built, nothing here ever downloads, and CPU tensors raise: there is no CPU fallback.  No trained checkpoint
has been available to check the loader against; the key naming is proven by loading this module's seeded state into WavLMModel with
strict=True (tests/golden/make_wavlm_fixtures.py)."""
from types import SimpleNamespace

import torch
from torch import nn

from lds import arch, native


class WavLM(nn.Module):
    def __init__(self, dims="base+", *, state=None, checkpoint=None, seed=None, normalize=None):
        """`dims`: "base+" / "large" or the fields of lds_wavlm_cfg.  The weights come from exactly one of `state` (a state dict in
        transformers naming), `checkpoint` (a local file holding one: load_checkpoint_state) or `seed` (lds.arch.wavlm_init_state: no
        checkpoint ships).  `normalize`: every clip is set to zero mean and unit variance first, on the device; None = as the published
        feature extractors do it (Large: yes, Base+: no)."""
        super().__init__()
        self.dims = arch.wavlm_dims(dims) if isinstance(dims, str) else {k: int(dims[k]) for k in native.WavLM.FIELDS}
        native.WavLM.check_dims(self.dims)
        if sum(v is not None for v in (state, checkpoint, seed)) != 1:
            raise ValueError("WavLM: pass exactly one of state=, checkpoint=PATH or seed= (nothing is downloaded)")
        self.normalize = bool(self.dims["stable_layer_norm"]) if normalize is None else bool(normalize)
        self._names = {}
        for k, s in arch.wavlm_param_shapes(self.dims).items():
            self._names[k] = k.replace(".", "__")      # (flat: "layers.0.attention" is no legal parameter name)
            self.register_parameter(self._names[k], nn.Parameter(torch.zeros(s), requires_grad=False))
        self._native = None
        if checkpoint is not None:
            state = load_checkpoint_state(checkpoint)
        elif seed is not None:
            state = arch.wavlm_init_state(self.dims, int(seed))
        self.load_state_dict(state)
        self.eval()

    def state_dict(self, *a, **k):
        sd = super().state_dict(*a, **k)
        return type(sd)((name, sd[flat]) for name, flat in self._names.items())

    def load_state_dict(self, state_dict, strict=True):
        """state_dict: transformers naming (lds.arch.wavlm_convert_state); every tensor of the network must be there (a missing one is a
        KeyError naming it); masked_spec_embed and the task heads are dropped"""
        self._native = None      # (new weights: the packed copy is rebuilt on the next call)
        conv = arch.wavlm_convert_state(state_dict, self.dims)
        return super().load_state_dict({self._names[k]: torch.as_tensor(v) for k, v in conv.items()}, strict=strict)

    def native(self):
        if self._native is None:
            self._native = native.WavLM(self.dims, {k: v.detach().cpu() for k, v in self.state_dict().items()})
        return self._native

    def _wave(self, name, x):
        if self.training:
            raise NotImplementedError(f"{name}: the training path (dropout, layer drop, masking) is not built; call .eval()")
        if not torch.is_tensor(x) or not x.is_cuda:
            raise RuntimeError(f"{name} needs the waveform as a tensor on a HIP device (no CPU fallback)")
        if x.dim() != 2:
            raise ValueError(f"{name}: waveform must be [B, L], got {list(x.shape)}")
        return x.float().contiguous()

    @torch.no_grad()
    def encode(self, wave, lengths=None, layer=None, layer_weights=None):
        """wave [B, L] at 16 kHz on a HIP device -> hidden_states[layer] [B, T, n_state] (None = last_hidden_state); `lengths`: every
        clip's own sample count, each clip encoded as if alone.  layer_weights (n_layer + 1 soft-maxed numbers): the weighted sum of all
        hidden states in one encode, what a *ForXVector head with use_weighted_layer_sum reads"""
        wave = self._wave("WavLM.encode", wave)      # (judged before a handle is built)
        return self.native().encode(wave, lengths, layer=layer, normalize=self.normalize, layer_weights=layer_weights)

    @torch.no_grad()
    def extract_features(self, wave, lengths=None):
        """-> feature_extractor(wave) transposed, [B, T, conv_dim]"""
        wave = self._wave("WavLM.extract_features", wave)
        return self.native().features(wave, lengths, normalize=self.normalize)

    @torch.no_grad()
    def forward(self, input_values, attention_mask=None, mask_time_indices=None, output_hidden_states=False, lengths=None):
        """WavLMModel.forward in inference: input_values [B, L] on a HIP device -> an object with `last_hidden_state` [B, T, n_state] and
        `hidden_states` (None, or with output_hidden_states the n_layer + 1 tensors, each a run of its own).  attention_mask must be None or
        all ones; `lengths` (not in transformers) gives every clip's own sample count instead."""
        if mask_time_indices is not None:
            raise NotImplementedError("WavLM: masking (mask_time_indices, SpecAugment) is the training path; not built")
        if attention_mask is not None and not bool(torch.as_tensor(attention_mask).bool().all()):
            raise NotImplementedError("WavLM: an attention_mask with zeros is not built; pass lengths= instead")
        wave = self._wave("WavLM.forward", input_values)
        hs = None
        if output_hidden_states:
            hs = tuple(self.native().encode(wave, lengths, layer=l, normalize=self.normalize) for l in range(self.dims["n_layer"] + 1))
        last = hs[-1] if hs is not None else self.native().encode(wave, lengths, normalize=self.normalize)
        return SimpleNamespace(last_hidden_state=last, hidden_states=hs)


def load_checkpoint_state(checkpoint):
    """The state dict of a local WavLM checkpoint in transformers naming: a `.safetensors` file (when `safetensors` imports) or a
    torch-saved dict of tensors, bare or under "state_dict" / "model", read with torch.load(weights_only=True)."""
    from encoder.wav2vec2_bert.model import load_checkpoint_state as load
    return load(checkpoint)
