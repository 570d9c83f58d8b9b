"""wav2vec 2.0 in its layer-norm flavour (XLSR-53) as a parameter holder over the native handle: the network that the reference's
tools/tools.py Audio2xlsr_53_56k loads through fairseq and runs as extract_features(source, padding_mask=all False)["x"].  The module
carries the tensors inference reads under fairseq's names (lds.arch.w2v_param_shapes); `extract_features` runs lds_w2v_encode.  The
quantiser, the masking and the training path are not built, nothing here ever downloads, and CPU tensors raise: there is no CPU
fallback.  The fairseq naming follows fairseq's published module layout and has not been checked against a real checkpoint file."""
import torch
from torch import nn

from lds import arch, native


class Wav2Vec2(nn.Module):
    def __init__(self, dims=None):
        """`dims`: the fields of lds.arch.XLSR_53_DIMS"""
        super().__init__()
        self.dims = dict(arch.XLSR_53_DIMS if dims is None else dims)
        native.Wav2Vec2.check_dims(self.dims)
        self._names = {}
        for k, s in arch.w2v_param_shapes(self.dims).items():
            self._names[k] = k.replace(".", "__")      # (flat: "conv_layers.0.2.1" is no legal module path)
            self.register_parameter(self._names[k], nn.Parameter(torch.zeros(s), requires_grad=False))
        self._native = None

    def state_dict(self, *a, **k):
        sd = super().state_dict(*a, **k)
        return type(sd)((name, sd[flat]) for name, flat in self._names.items())

    def load_state_dict(self, state_dict, strict=True):
        """state_dict: fairseq or transformers naming (lds.arch.w2v_convert_state); every tensor of the network must be there"""
        self._native = None      # (new weights: the packed copy is rebuilt on the next call)
        conv = arch.w2v_convert_state(state_dict, self.dims)
        return super().load_state_dict({self._names[k]: torch.as_tensor(v) for k, v in conv.items()}, strict=strict)

    def native(self):
        if self._native is None:
            self._native = native.Wav2Vec2(self.dims, {k: v.detach().cpu() for k, v in self.state_dict().items()})
        return self._native

    @staticmethod
    def _wave(name, x):
        if not torch.is_tensor(x) or not x.is_cuda:
            raise RuntimeError(f"{name} needs the waveform as a tensor on a HIP device (no CPU fallback)")
        if x.dim() != 2:
            raise ValueError(f"{name}: waveform must be [B, L], got {list(x.shape)}")
        return x.float().contiguous()

    @torch.no_grad()
    def extract_features(self, source, padding_mask=None, mask=False, lengths=None):
        """source [B, L] on a HIP device -> {"x": [B, T, n_state], "padding_mask": None}.  padding_mask must be None or all False (the
        reference passes all False); `lengths` (not in fairseq): every clip's own sample count, each clip encoded as if alone."""
        wave = self._wave("Wav2Vec2.extract_features", source)
        if mask:
            raise NotImplementedError("Wav2Vec2: masking is the training path; not built")
        if padding_mask is not None and bool(torch.as_tensor(padding_mask).any()):
            raise NotImplementedError("Wav2Vec2: a padding_mask with True entries is not built; pass lengths= instead")
        return {"x": self.native().encode(wave, lengths), "padding_mask": None}

    def forward(self, *a, **k):
        raise NotImplementedError("Wav2Vec2.forward is the training path (quantiser, masking, contrastive logits); not built: use extract_features")


def load_checkpoint_state(checkpoint):
    """The state dict of a local wav2vec 2.0 checkpoint: a bare dict of tensors or one under "model" (fairseq's layout), read with
    torch.load(weights_only=True) first.  A fairseq checkpoint whose pickle needs fairseq's classes (its "cfg" / "args") cannot be read
    without fairseq: the error says how to re-save the "model" dict alone."""
    import pickle
    try:
        ck = torch.load(checkpoint, map_location="cpu", weights_only=True)
    except (pickle.UnpicklingError, RuntimeError, AttributeError, ModuleNotFoundError) as e:
        raise RuntimeError(
            f"{checkpoint}: not readable as plain tensors ({type(e).__name__}: {str(e).splitlines()[0][:200]}).  A fairseq checkpoint pickles "
            "fairseq's own configuration classes next to the weights; on a machine with fairseq, re-save the weights alone: "
            "torch.save({'model': torch.load(PATH, weights_only=False)['model']}, NEW_PATH), and pass NEW_PATH") from e
    if isinstance(ck, dict) and isinstance(ck.get("model"), dict):
        ck = ck["model"]
    if not isinstance(ck, dict) or not all(torch.is_tensor(v) for v in ck.values()):
        raise RuntimeError(f"{checkpoint}: expected a state dict of tensors, bare or under 'model'")
    return ck
