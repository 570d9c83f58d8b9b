"""HuBERT-base / HuBERT-Soft / HuBERT-Discrete as parameter holders over the native handle (reference encoder/hubert/model.py:19-269).
The classes take the reference's constructor arguments and carry exactly its `state_dict` keys -- the unused `masked_spec_embed` and
`label_embedding.weight` included -- so a reference checkpoint loads with strict=True; `encode` / `units` run lds_hubert_encode.  The
training path (`mask`, `logits`, `forward`) is not built, nothing here ever downloads, and CPU tensors raise: there is no CPU fallback."""
from typing import Optional, Tuple

import torch
from torch import nn

from lds import arch, native


class Hubert(nn.Module):
    def __init__(self, num_label_embeddings: int = 100, mask: bool = True, *, dims=None):
        """`dims` (keyword-only, not in the reference, whose widths are literals): the fields of lds.arch.HUBERT_BASE_DIMS"""
        super().__init__()
        self._mask = mask
        self.dims = dict(arch.HUBERT_BASE_DIMS if dims is None else dims)
        native.Hubert.check_dims(self.dims)
        for k, s in arch.hubert_param_shapes(self.dims, num_label_embeddings).items():
            self._register(k, torch.zeros(s))
        self._native = None

    def _register(self, name, value):
        mod = self
        parts = name.split(".")
        for p in parts[:-1]:
            if not hasattr(mod, p):
                mod.add_module(p, nn.Module())
            mod = getattr(mod, p)
        mod.register_parameter(parts[-1], nn.Parameter(value, requires_grad=False))

    def load_state_dict(self, state_dict, *a, **k):
        self._native = None      # (new weights: the packed copy is rebuilt on the next call)
        return super().load_state_dict(state_dict, *a, **k)

    def native(self):
        if self._native is None:
            self._native = native.Hubert(self.dims, {k: v.detach().cpu() for k, v in self.state_dict().items()})
        return self._native

    def _wave(self, name, x):
        if not torch.is_tensor(x) or not x.is_cuda:
            raise RuntimeError(f"{name} needs the waveform as a tensor on a HIP device (no CPU fallback)")
        if x.dim() != 3 or x.shape[1] != 1:
            raise ValueError(f"{name}: waveform must be [B, 1, L], got {list(x.shape)}")
        return x[:, 0].float().contiguous()

    def mask(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        raise NotImplementedError("Hubert.mask is the training path (SpecAugment spans); not built")

    @torch.no_grad()
    def encode(self, x: torch.Tensor, layer: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """x [B, 1, L] on a HIP device, taken as it is (no padding: `units` pads) -> ([B, T, n_state], None): the output of the first
        `layer` blocks (None: all, 0: the output of `norm`); T = ((L - 400) // 320) + 1.  Every row of the batch is encoded as if alone."""
        wave = self._wave("Hubert.encode", x)      # (refused before the weights go to a device)
        return self.native().encode(wave, layer=layer, pad=0), None

    def logits(self, x: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError("Hubert.logits is the training path; not built")

    def forward(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        raise NotImplementedError("Hubert.forward is the training path (masked prediction logits); not built: use encode / units")


class HubertSoft(Hubert):
    def __init__(self, *, dims=None):
        super().__init__(dims=dims)

    @torch.inference_mode()
    def units(self, wav: torch.Tensor) -> torch.Tensor:
        """wav [B, 1, L] -> soft units [B, L // 320, n_proj]: proj(encode(pad(wav, 40, 40)))"""
        wave = self._wave("HubertSoft.units", wav)
        return self.native().encode(wave, proj=True, pad=arch.HUBERT_PAD)

    @torch.inference_mode()
    def units_ragged(self, wav: torch.Tensor, lengths, layer: Optional[int] = None, proj: bool = True):
        """Extension (not in the reference): wav [B, L] padded to the longest clip + every clip's own sample count (host ints, 320 .. L, at
        most 64 clips) -> (units [B, L // 320, n_proj], n_frames int64 [B] on the host): every clip as `units` gives it alone, zero rows
        beyond its own lengths[b] // 320.  proj=False with `layer`: the transformer's output after that many blocks instead."""
        if wav.dim() != 2:
            raise ValueError(f"HubertSoft.units_ragged: wav must be [B, L], got {list(wav.shape)}")
        ln = native.Hubert.lengths(lengths, wav.shape[0], wav.shape[1])      # (host-side validation first: a bad length is a ValueError on any device)
        if not wav.is_cuda:
            raise RuntimeError("HubertSoft.units_ragged needs the waveform on a HIP device (no CPU fallback)")
        u = self.native().encode(wav.float().contiguous(), ln, layer=layer, proj=proj)
        return u, torch.from_numpy(ln.astype("int64") // arch.HUBERT_HOP)


class HubertDiscrete(Hubert):
    def __init__(self, kmeans, *, dims=None):
        """kmeans: a codebook for cluster.get_cluster_result (a model from cluster.get_cluster_model, or anything with the scikit-learn
        attribute `cluster_centers_`); None until one is attached"""
        super().__init__(504, dims=dims)
        self.kmeans = kmeans

    @torch.inference_mode()
    def units(self, wav: torch.Tensor) -> torch.LongTensor:
        """wav [1, 1, L] -> int64 [L // 320] on the device: the nearest centre of encode(pad(wav), layer=7) by lds_kmeans_assign"""
        import cluster
        if self.kmeans is None:
            raise RuntimeError("HubertDiscrete.units needs a codebook (kmeans)")
        wave = self._wave("HubertDiscrete.units", wav)
        x = self.native().encode(wave, layer=7, pad=arch.HUBERT_PAD)
        return cluster.get_cluster_result(self.kmeans, x.reshape(-1, x.shape[-1]))


def _load(model, checkpoint):
    state = torch.load(checkpoint, map_location="cpu", weights_only=False)
    state = state.get("model_state_dict", state) if isinstance(state, dict) else state
    nn.modules.utils.consume_prefix_in_state_dict_if_present(state, "module.")
    model.load_state_dict(state)
    return model.eval()


def hubert_soft(pretrained: bool = True, progress: bool = True, *, checkpoint=None) -> HubertSoft:
    """The reference downloads the weights; nothing here fetches: pass `checkpoint=PATH` (keyword-only), a local file holding the
    reference's state dict, or pretrained=False for an empty model."""
    if checkpoint is not None:
        return _load(HubertSoft(), checkpoint)
    if pretrained:
        raise NotImplementedError("hubert_soft(pretrained=True) would download; pass checkpoint=PATH (a local state dict) instead")
    return HubertSoft()


def hubert_discrete(pretrained: bool = True, progress: bool = True, *, checkpoint=None, kmeans=None) -> HubertDiscrete:
    """As hubert_soft; `kmeans` = the codebook (the reference downloads that too)"""
    if checkpoint is not None:
        return _load(HubertDiscrete(kmeans), checkpoint)
    if pretrained:
        raise NotImplementedError("hubert_discrete(pretrained=True) would download; pass checkpoint=PATH (a local state dict) and kmeans= instead")
    return HubertDiscrete(kmeans)
