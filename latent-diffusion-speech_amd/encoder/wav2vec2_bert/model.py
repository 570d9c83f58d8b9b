"""w2v-BERT 2.0 as a parameter holder over the native handle: the network that the reference's tools/tools.py Wav2Vec2Bert loads with
transformers' Wav2Vec2BertModel.from_pretrained("facebook/w2v-bert-2.0") and runs on SeamlessM4TFeatureExtractor's output.  The module
carries the tensors inference reads under transformers' names (lds.arch.w2vbert_param_shapes); `forward` runs lds_w2vbert_encode_features,
`encode_audio` the filter bank and the model in one call.  The adapter, the masking and the training heads are not built, nothing here
ever downloads, and CPU tensors raise: there is no CPU fallback.  No trained checkpoint has been available to check the loader against."""
import torch
from torch import nn

from lds import arch, native


class Wav2Vec2BertModel(nn.Module):
    def __init__(self, dims=None):
        """`dims`: the fields of lds.arch.W2V_BERT_DIMS"""
        super().__init__()
        self.dims = native.Wav2Vec2Bert.check_dims(dict(arch.W2V_BERT_DIMS if dims is None else dims))
        self._names = {}
        for k, s in arch.w2vbert_param_shapes(self.dims).items():
            self._names[k] = k.replace(".", "__")      # (flat: "layers.0.ffn1" is no legal parameter name)
            self.register_parameter(self._names[k], nn.Parameter(torch.zeros(s), requires_grad=False))
        self._native = None

    def state_dict(self, *a, **k):
        sd = super().state_dict(*a, **k)
        return type(sd)((name, sd[flat]) for name, flat in self._names.items())

    def load_state_dict(self, state_dict, strict=True):
        """state_dict: transformers naming (lds.arch.w2vbert_convert_state); every tensor of the network must be there (a missing one is a
        KeyError naming it); masked_spec_embed is dropped"""
        self._native = None      # (new weights: the packed copy is rebuilt on the next call)
        conv = arch.w2vbert_convert_state(state_dict, self.dims)
        return super().load_state_dict({self._names[k]: torch.as_tensor(v) for k, v in conv.items()}, strict=strict)

    def native(self):
        if self._native is None:
            self._native = native.Wav2Vec2Bert(self.dims, {k: v.detach().cpu() for k, v in self.state_dict().items()})
        return self._native

    @staticmethod
    def _on_device(name, x, ndim, what):
        if not torch.is_tensor(x) or not x.is_cuda:
            raise RuntimeError(f"{name} needs {what} as a tensor on a HIP device (no CPU fallback)")
        if x.dim() != ndim:
            raise ValueError(f"{name}: {what} must have {ndim} dimensions, got {list(x.shape)}")
        return x.float().contiguous()

    @torch.no_grad()
    def forward(self, input_features, attention_mask=None):
        """input_features [B, R, 160] on a HIP device, attention_mask [B, R] of ones followed by zeros (the extractor's) or None ->
        last_hidden_state [B, R, n_state], masked rows included (computed as the reference computes them).  Rows behind a clip's first
        masked row are zeros here."""
        f = self._on_device("Wav2Vec2BertModel.forward", input_features, 3, "input_features")
        n = None
        if attention_mask is not None:
            m = torch.as_tensor(attention_mask).cpu().long()
            valid = m.sum(-1)
            if not bool((m == (torch.arange(m.shape[1])[None] < valid[:, None]).long()).all()):
                raise NotImplementedError("Wav2Vec2BertModel: attention_mask must be ones followed by zeros")
            st = self.dims["stride"]
            n = [min(int(v) * st + (st - 1 if int(v) < m.shape[1] else 0), st * m.shape[1]) for v in valid]      # rows = min(valid + 1, R)
        return self.native().encode_features(f, n)

    @torch.no_grad()
    def encode_audio(self, audio, lengths=None):
        """audio [B, L] at 16 kHz on a HIP device -> last_hidden_state [B, R, n_state] (filter bank + model); `lengths`: every clip's own
        sample count, each clip encoded as if alone"""
        wave = self._on_device("Wav2Vec2BertModel.encode_audio", audio, 2, "the waveform")      # (judged before a handle is built)
        return self.native().encode(wave, lengths)


def load_checkpoint_state(checkpoint):
    """The state dict of a local w2v-BERT checkpoint in transformers naming: a `.safetensors` file (when `safetensors` imports) or a
    torch-saved dict of tensors, bare or under "state_dict" / "model", read with torch.load(weights_only=True)."""
    import pickle
    if str(checkpoint).endswith(".safetensors"):
        try:
            from safetensors.torch import load_file
        except ImportError as e:
            raise RuntimeError(f"{checkpoint}: reading .safetensors needs the safetensors package; re-save the state dict with torch.save") from e
        return load_file(str(checkpoint), device="cpu")
    try:
        ck = torch.load(checkpoint, map_location="cpu", weights_only=True)
    except (pickle.UnpicklingError, RuntimeError, AttributeError, ModuleNotFoundError) as e:
        raise RuntimeError(f"{checkpoint}: not readable as plain tensors ({type(e).__name__}: {str(e).splitlines()[0][:200]}); "
                           "save model.state_dict() alone with torch.save") from e
    for key in ("state_dict", "model"):
        if isinstance(ck, dict) and isinstance(ck.get(key), dict):
            ck = ck[key]
    if not isinstance(ck, dict) or not all(torch.is_tensor(v) for v in ck.values()):
        raise RuntimeError(f"{checkpoint}: expected a state dict of tensors, bare or under 'state_dict' / 'model'")
    return ck
