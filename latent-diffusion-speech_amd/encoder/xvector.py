"""x-vector speaker embeddings on the speech encoders (transformers' WavLMForXVector / Wav2Vec2ForXVector: projector, TDNN layers,
statistics pooling, feature_extractor, classifier; e.g. microsoft/wavlm-base-plus-sv).  XVectorHead holds the head's weights on the device
and runs csrc/xvector.hip over (hidden [B, T, D], n_frames [B]) -- the pair that every units encoder's `encode_ragged` returns;
SpeakerEncoder puts it behind a WavLMUnits: audio -> embeddings, and the cosine of two embeddings is the speaker similarity that TTS and
voice-conversion work reports next to the error rate (include/lds.h lds_xvector_*).  There is no CPU path: CPU tensors raise.

Every clip is embedded as if given alone with attention_mask=None, the project's rule everywhere.  transformers' batched attention_mask
path is NOT reproduced: its _get_tdnn_output_lengths ignores the dilations (it pools T - 8 frames of a tensor that holds T - 14 valid
ones) and the Base encoder's group norm sees the padding.

Which hidden states a head reads: with `layer_weights` (config.use_weighted_layer_sum) the soft-max weighted sum of ALL n_layer + 1 hidden
states (WavLM.encode(layer_weights=), one encode); otherwise the last hidden state.  The head itself is encoder-agnostic; only the
layer-sum entry is WavLM's.  Not built: the AM-softmax loss (`objective.*`, training), clips above the encoder's 30 s window."""
import json
import os

import numpy as np
import torch

from lds import arch, init_weights, native

from .ctc import ENCODER_PREFIXES, _load_state

HEAD_PREFIXES = ("projector.", "tdnn.", "feature_extractor.", "classifier.", "objective.")
HEAD_KEYS = ("layer_weights",)
DEFAULT_TDNN = arch.XVECTOR_GEOMETRY


def load_xvector_encoder_state(path_or_state):
    """the encoder half of a *ForXVector checkpoint (a path or a state dict): the `wavlm.` / `wav2vec2.` / `hubert.` prefix is stripped FIRST,
    then the head's top-level keys are dropped -- in that order, because the head's `feature_extractor.{weight,bias}` and the encoder's
    `wavlm.feature_extractor.conv_layers.*` differ only by the prefix"""
    state = path_or_state if isinstance(path_or_state, dict) else _load_state(path_or_state)
    out, seen = {}, set()
    for k, v in state.items():
        for p in ENCODER_PREFIXES:
            if k.startswith(p):
                seen.add(p)
                out[k[len(p):]] = v
                break
        else:
            if not (k in HEAD_KEYS or k.startswith(HEAD_PREFIXES)):
                out[k] = v
    if len(seen) > 1:
        raise ValueError(f"load_xvector_encoder_state: keys under more than one encoder prefix {sorted(seen)}")
    return out


def softmax64(w):
    w = np.asarray(w, dtype=np.float64)
    e = np.exp(w - w.max())
    return e / e.sum()


class XVectorHead:
    """The head of a *ForXVector model.  `state`: projector.{weight,bias}, tdnn.{i}.kernel.{weight,bias}, feature_extractor.{weight,bias},
    classifier.{weight,bias} (any float arrays / tensors) and optionally layer_weights [n_layer + 1] (raw, as stored: soft-maxed here in
    float64); the geometry is HF's config keys."""

    def __init__(self, state, tdnn_dim=DEFAULT_TDNN["tdnn_dim"], tdnn_kernel=DEFAULT_TDNN["tdnn_kernel"], tdnn_dilation=DEFAULT_TDNN["tdnn_dilation"],
                 xvector_output_dim=DEFAULT_TDNN["xvector_output_dim"], device="cuda"):
        st = {k: np.asarray(v.detach().cpu() if torch.is_tensor(v) else v, dtype=np.float32) for k, v in state.items()
              if k in HEAD_KEYS or (k.startswith(HEAD_PREFIXES) and not k.startswith("objective."))}
        if "projector.weight" not in st or st["projector.weight"].ndim != 2:
            raise ValueError("XVectorHead: the state holds no projector.weight [tdnn_dim[0], D]")
        self.tdnn_dim, self.tdnn_kernel, self.tdnn_dilation = tuple(int(v) for v in tdnn_dim), tuple(int(v) for v in tdnn_kernel), tuple(int(v) for v in tdnn_dilation)
        self.D, self.xvector_dim, self.device = int(st["projector.weight"].shape[1]), int(xvector_output_dim), device
        if st["projector.weight"].shape[0] != self.tdnn_dim[0]:
            raise ValueError(f"XVectorHead: projector.weight {list(st['projector.weight'].shape)} against tdnn_dim[0] = {self.tdnn_dim[0]}")
        self.span = sum((k - 1) * d for k, d in zip(self.tdnn_kernel, self.tdnn_dilation))
        self.min_frames = self.span + 2
        lw = st.pop("layer_weights", None)
        self.layer_weights = None if lw is None else softmax64(lw.reshape(-1)).astype(np.float32)
        need = ["projector.weight", "projector.bias", "feature_extractor.weight", "feature_extractor.bias", "classifier.weight", "classifier.bias"]
        need += [f"tdnn.{i}.kernel.{w}" for i in range(len(self.tdnn_dim)) for w in ("weight", "bias")]
        missing = [k for k in need if k not in st]
        if missing:
            raise ValueError(f"XVectorHead: the state lacks {missing}")
        # the geometry is judged here (ValueError, no device needed); the handle is built on first use
        native.xvector_check_layer(self.D, self.tdnn_dim[0], 1, 1, "XVectorHead projector")
        for i in range(len(self.tdnn_dim)):
            native.xvector_check_layer(self.tdnn_dim[i - 1] if i else self.tdnn_dim[0], self.tdnn_dim[i], self.tdnn_kernel[i], self.tdnn_dilation[i], f"XVectorHead tdnn.{i}")
        self._state, self._h = st, None
        self.n_labels = int(st["classifier.bias"].shape[0])

    # ---- construction ----
    @classmethod
    def synthetic(cls, D, seed=0, n_layer=None, n_labels=None, device="cuda", **geometry):
        """seeded weights (lds.init_weights): uniform in +- 1 / sqrt(fan_in), as torch.nn.Linear's default; n_layer: also seeded, non-uniform
        layer_weights over n_layer + 1 hidden states"""
        g = dict(DEFAULT_TDNN, **geometry)
        return cls(arch.xvector_init_state(D, seed, n_layer, n_labels, g, init_weights), device=device, **g)

    @classmethod
    def from_checkpoint(cls, path, device="cuda"):
        """a local transformers *ForXVector state dict (torch-saved or .safetensors) and, when present next to it, config.json's tdnn_dim /
        tdnn_kernel / tdnn_dilation / xvector_output_dim / use_weighted_layer_sum.  Nothing is downloaded."""
        state = _load_state(path)
        if "projector.weight" not in state:
            raise ValueError(f"XVectorHead.from_checkpoint: {path} holds no projector.weight")
        here = os.path.dirname(os.path.abspath(str(path)))
        g, use_sum = dict(DEFAULT_TDNN), "layer_weights" in state
        if os.path.exists(os.path.join(here, "config.json")):
            cfg = json.load(open(os.path.join(here, "config.json")))
            g.update({k: cfg[k] for k in DEFAULT_TDNN if k in cfg})
            use_sum = bool(cfg.get("use_weighted_layer_sum", use_sum))
        if use_sum and "layer_weights" not in state:
            raise ValueError(f"XVectorHead.from_checkpoint: use_weighted_layer_sum is set but {path} holds no layer_weights")
        head = {k: v for k, v in state.items() if not k.startswith(ENCODER_PREFIXES) and (use_sum or k != "layer_weights")}
        return cls(head, device=device, **g)

    # ---- which hidden states ----
    def check_source(self, encoder):
        """ValueError unless `encoder` (a Units_Encoder or one of its models) can feed this head: a WavLM whose depth matches layer_weights when
        the head sums the layers, else any encoder returning the last hidden state of a stack as wide as the head's input"""
        model = getattr(encoder, "model", encoder) if type(encoder).__name__ == "Units_Encoder" else encoder
        if getattr(model, "proj", False):
            raise ValueError("XVectorHead: 'hubertsoft' units are the 256-wide projection behind the last layer, not a hidden state")
        if type(model).__name__ in ("WhisperLargeV3", "Wav2Vec2Bert"):
            raise ValueError(f"XVectorHead: x-vector heads for {type(model).__name__} units are not built")
        dims = getattr(getattr(model, "model", None), "dims", None)
        if self.layer_weights is not None:
            if type(model).__name__ != "WavLMUnits":
                raise ValueError("XVectorHead: this head sums the hidden states (layer_weights); the layer-sum entry is WavLM's only")
            if len(self.layer_weights) != dims["n_layer"] + 1:
                raise ValueError(f"XVectorHead: {len(self.layer_weights)} layer_weights against an encoder of {dims['n_layer']} layers")
        else:
            layer = getattr(model, "units_layer", None)
            if layer is not None and dims is not None and layer != dims["n_layer"]:
                raise ValueError(f"XVectorHead: this WavLM returns hidden_states[{layer}] (units_layer is set); the head reads the last hidden state")
        if getattr(model, "hidden_dim", self.D) != self.D:
            raise ValueError(f"XVectorHead: a head over {self.D}-wide hidden states against a {model.hidden_dim}-wide encoder")

    def native(self):
        if self._h is None:
            self._h = native.XVector(self.D, self.tdnn_dim, self.tdnn_kernel, self.tdnn_dilation, self.xvector_dim, self._state)
        return self._h

    @torch.inference_mode()
    def embed(self, hidden, n_frames=None):
        """hidden [B, T, D] (or [T, D]) on a HIP device, n_frames [B] -> (embeddings [B, xvector_dim], logits [B, n_labels]) on the device"""
        if not torch.is_tensor(hidden) or not hidden.is_cuda:
            raise RuntimeError("XVectorHead needs the hidden states as a tensor on a HIP device (no CPU fallback)")
        if hidden.dim() == 2:
            hidden = hidden.unsqueeze(0)
        if hidden.dim() != 3 or hidden.shape[-1] != self.D:
            raise ValueError(f"XVectorHead: hidden states {list(hidden.shape)} against a head over {self.D}-wide ones")
        if n_frames is None:
            n_frames = [hidden.shape[1]] * hidden.shape[0]
        nf = np.asarray(n_frames.cpu() if torch.is_tensor(n_frames) else n_frames).reshape(-1)
        if len(nf) and nf.min() < self.min_frames:
            raise ValueError(f"XVectorHead: a clip of {int(nf.min())} frames leaves {max(int(nf.min()) - self.span, 0)} frames to pool; the unbiased "
                             f"standard deviation needs 2, i.e. at least {self.min_frames} frames")
        return self.native().embed(hidden.float().contiguous(), nf)


class SpeakerEncoder:
    """audio -> speaker embeddings: a WavLMUnits (tools.tools) and an XVectorHead.  `embed_audio` takes the layer-sum entry when the head has
    layer_weights and the last hidden state otherwise; `similarity` is the cosine of every pair."""

    def __init__(self, wavlm_units, head):
        head.check_source(wavlm_units)
        self.units, self.head = wavlm_units, head

    @torch.inference_mode()
    def embed_audio(self, audio, lengths=None, return_logits=False):
        """audio [B, L] at 16 kHz on a HIP device, lengths: every clip's own sample count (None: all L) -> embeddings [B, xvector_dim]
        (with return_logits: and the classifier's logits [B, n_labels])"""
        if not torch.is_tensor(audio) or not audio.is_cuda:
            raise RuntimeError("SpeakerEncoder needs the audio as a tensor on a HIP device (no CPU fallback)")
        if audio.dim() != 2:
            raise ValueError(f"SpeakerEncoder.embed_audio: audio must be [B, L], got {list(audio.shape)}")
        B, L = audio.shape
        ln = native.WavLM.lengths([L] * B if lengths is None else lengths, B, L)
        frames = np.array([self.units.frames_of(int(n)) for n in ln])
        if frames.min() < self.head.min_frames:
            raise ValueError(f"SpeakerEncoder: a clip of {int(ln[frames.argmin()])} samples gives {int(frames.min())} frames; the head needs "
                             f"{self.head.min_frames} (5,200 samples with the default geometry)")
        model = self.units.model
        hidden = model.encode(audio.float().contiguous(), ln, layer_weights=self.head.layer_weights)
        emb, logits = self.head.embed(hidden, frames)
        return (emb, logits) if return_logits else emb

    @staticmethod
    @torch.inference_mode()
    def similarity(a, b):
        """embeddings a [N, dim], b [M, dim] on a HIP device -> cosine similarities [N, M]"""
        for t in (a, b):
            if not torch.is_tensor(t) or not t.is_cuda:
                raise RuntimeError("SpeakerEncoder.similarity needs the embeddings on a HIP device (no CPU fallback)")
        a, b = (t.unsqueeze(0) if t.dim() == 1 else t for t in (a, b))
        return native.xvector_cosine(a.float().contiguous(), b.float().contiguous())


def equal_error_rate(scores, labels):
    """the EER of similarity scores against 0 / 1 labels (1 = same speaker): the point where the false-accept and false-reject rates cross,
    the mean of the two at the threshold where their difference is smallest"""
    s, y = np.asarray(scores, dtype=np.float64), np.asarray(labels).astype(bool)
    if y.all() or not y.any():
        raise ValueError("equal_error_rate needs both same-speaker and different-speaker pairs")
    best = (2.0, 0.5)
    for th in np.unique(s):
        far, frr = float((s[~y] >= th).mean()), float((s[y] < th).mean())
        if abs(far - frr) < best[0]:
            best = (abs(far - frr), 0.5 * (far + frr))
    return best[1]
