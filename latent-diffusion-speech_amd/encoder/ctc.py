"""CTC heads on the speech encoders (transformers' Wav2Vec2ForCTC / HubertForCTC / WavLMForCTC: `lm_head` over the last hidden state).
CTCHead holds lm_head's weight [V, D] and bias [V] on the device and runs csrc/ctc.hip over (units [B, T, D], n_frames [B]) -- the pair
that every units encoder's `encode_ragged` returns: log-probs, the greedy transcript, the CTC score of a given transcript and its forced
alignment (include/lds.h lds_ctc_*).  There is no CPU path: CPU tensors raise.

Which units a head applies to: the LAST hidden state of the stack the head was trained on -- 'xlsr_53_56k', 'wavlmbase+' / 'wavlmlarge' with
units_layer=None, 'contentvec768l12'.  'hubertsoft' units are the 256-wide projection behind the last layer and a WavLM with units_layer
set returns an inner layer: `check_source` refuses both with a ValueError naming the reason."""
import json
import os

import numpy as np
import torch

from lds import init_weights, native

ENCODER_PREFIXES = ("wav2vec2.", "wavlm.", "hubert.")
MAX_LABELS = native.CTC_MAX_LABELS


def _load_state(path):
    """a local transformers state dict: .safetensors, or torch-saved plain tensors (bare or under "state_dict" / "model")"""
    if str(path).endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(str(path))
    state = torch.load(path, map_location="cpu", weights_only=False)
    for k in ("state_dict", "model"):
        if isinstance(state, dict) and k in state and isinstance(state[k], dict):
            state = state[k]
    return state


def load_ctc_encoder_state(path_or_state):
    """the encoder half of a *ForCTC checkpoint (a path or a state dict): the `wav2vec2.` / `wavlm.` / `hubert.` prefix stripped and lm_head.*
    dropped, so that the loaders of Audio2xlsr_53_56k / WavLMUnits / HubertUnits take a fine-tuned checkpoint's encoder"""
    state = path_or_state if isinstance(path_or_state, dict) else _load_state(path_or_state)
    out, seen = {}, set()
    for k, v in state.items():
        if k.startswith("lm_head."):
            continue
        for p in ENCODER_PREFIXES:
            if k.startswith(p):
                seen.add(p)
                k = k[len(p):]
                break
        out[k] = v
    if len(seen) > 1:
        raise ValueError(f"load_ctc_encoder_state: keys under more than one encoder prefix {sorted(seen)}")
    return out


class CTCHead:
    """lm_head of a *ForCTC model.  weight [V, D], bias [V] (any float arrays / tensors; kept as fp32 on `device`), blank = HF's
    config.pad_token_id, vocab = HF's vocab.json ({token: id}) or None."""

    def __init__(self, weight, bias, blank=0, vocab=None, device="cuda"):
        w = torch.as_tensor(np.asarray(weight.detach().cpu() if torch.is_tensor(weight) else weight), dtype=torch.float32)
        b = torch.as_tensor(np.asarray(bias.detach().cpu() if torch.is_tensor(bias) else bias), dtype=torch.float32)
        if w.dim() != 2 or b.shape != (w.shape[0],):
            raise ValueError(f"CTCHead: weight {list(w.shape)} and bias {list(b.shape)} are not [V, D] and [V]")
        V, D = w.shape
        if D < 8 or D > 4096 or D % 8:
            raise ValueError(f"CTCHead: D {D} must be a multiple of 8 in 8 .. 4096")
        if V < 2 or V > 65536:
            raise ValueError(f"CTCHead: V {V} outside 2 .. 65536")
        if not 0 <= int(blank) < V:
            raise ValueError(f"CTCHead: blank {blank} outside 0 .. {V - 1}")
        self.V, self.D, self.blank, self.device = V, D, int(blank), device
        self._w, self._b, self._on = w.contiguous(), b.contiguous(), None
        self.vocab = None
        if vocab is not None:
            self.vocab = {int(i): t for t, i in vocab.items()}

    # ---- construction ----
    @classmethod
    def synthetic(cls, D, V, seed=0, blank=0, device="cuda"):
        """seeded weights (lds.init_weights): uniform in +- 1 / sqrt(D), as torch.nn.Linear's default"""
        k = 1.0 / np.sqrt(D)
        return cls(init_weights.uniform("lm_head.weight", (V, D), seed, -k, k), init_weights.uniform("lm_head.bias", (V,), seed, -k, k), blank, device=device)

    @classmethod
    def from_checkpoint(cls, path, device="cuda"):
        """a local transformers *ForCTC state dict (torch-saved or .safetensors): lm_head.* and, when present next to it, config.json's
        pad_token_id and vocab.json.  Nothing is downloaded."""
        state = _load_state(path)
        if "lm_head.weight" not in state or "lm_head.bias" not in state:
            raise ValueError(f"CTCHead.from_checkpoint: {path} holds no lm_head.weight / lm_head.bias")
        here = os.path.dirname(os.path.abspath(str(path)))
        blank, vocab = 0, None
        if os.path.exists(os.path.join(here, "config.json")):
            blank = json.load(open(os.path.join(here, "config.json"))).get("pad_token_id", 0) or 0
        if os.path.exists(os.path.join(here, "vocab.json")):
            vocab = json.load(open(os.path.join(here, "vocab.json")))
        return cls(state["lm_head.weight"], state["lm_head.bias"], blank, vocab, device=device)

    # ---- which units ----
    @staticmethod
    def check_source(encoder):
        """ValueError unless `encoder` (a Units_Encoder or one of its models) returns the last hidden state of its stack"""
        model = getattr(encoder, "model", encoder) if type(encoder).__name__ == "Units_Encoder" else encoder
        if getattr(model, "proj", False):
            raise ValueError("CTCHead: 'hubertsoft' units are the 256-wide projection behind the last layer, not the hidden state a CTC head "
                             "reads; use 'contentvec768l12' (the last layer of the same stack)")
        layer = getattr(model, "units_layer", None)
        if layer is not None and layer != model.model.dims["n_layer"]:
            raise ValueError(f"CTCHead: this WavLM returns hidden_states[{layer}] (units_layer is set); a CTC head reads the last hidden state "
                             "(units_layer=None)")
        if type(model).__name__ in ("WhisperLargeV3", "Wav2Vec2Bert"):
            raise ValueError(f"CTCHead: CTC heads for {type(model).__name__} units are not built")

    def _args(self, units, n_frames):
        if not torch.is_tensor(units) or not units.is_cuda:
            raise RuntimeError("CTCHead needs the units as a tensor on a HIP device (no CPU fallback)")
        if units.dim() == 2:
            units = units.unsqueeze(0)
        if units.dim() != 3 or units.shape[-1] != self.D:
            raise ValueError(f"CTCHead: units {list(units.shape)} against a head over {self.D}-wide hidden states")
        if n_frames is None:
            n_frames = [units.shape[1]] * units.shape[0]
        if self._on != units.device:
            self._wd, self._bd, self._on = self._w.to(units.device), self._b.to(units.device), units.device
        return units.float().contiguous(), n_frames

    def _labels(self, labels, B):
        """a list of B id sequences (or an int array [B, L] with label_len) -> (padded int64 [B, Lmax] on the host, lengths); ids are checked here"""
        seqs = [np.asarray(s.cpu() if torch.is_tensor(s) else s, dtype=np.int64).reshape(-1) for s in labels]
        if len(seqs) != B:
            raise ValueError(f"CTCHead: {len(seqs)} transcripts for {B} clips")
        Lmax = max([len(s) for s in seqs] + [1])
        if Lmax > MAX_LABELS:
            raise ValueError(f"CTCHead: at most {MAX_LABELS} labels per clip (got {Lmax})")
        pad = np.zeros((B, Lmax), dtype=np.int64)
        for b, s in enumerate(seqs):
            if len(s) and (s.min() < 0 or s.max() >= self.V):
                raise ValueError(f"CTCHead: clip {b} has a label outside 0 .. {self.V - 1}")
            if (s == self.blank).any():
                raise ValueError(f"CTCHead: clip {b} has the blank ({self.blank}) as a label")
            pad[b, :len(s)] = s
        return pad, np.array([len(s) for s in seqs], dtype=np.int32)

    # ---- the four calls ----
    @torch.inference_mode()
    def log_probs(self, units, n_frames=None):
        """-> log-probs [B, T, V] (zeros at and beyond a clip's n_frames): HF's .logits.log_softmax(-1)"""
        units, n_frames = self._args(units, n_frames)
        return native.ctc_head(units, n_frames, self._wd, self._bd, return_logprobs=True)[3]

    @torch.inference_mode()
    def greedy(self, units, n_frames=None):
        """-> one dict per clip: tokens, start, length (frames) as int arrays and logprob (the mean log-prob of each token's run), on the host"""
        units, n_frames = self._args(units, n_frames)
        arg, m, lse = native.ctc_head(units, n_frames, self._wd, self._bd)
        tok, n, start, length, lp = (t.cpu().numpy() for t in native.ctc_greedy(arg, m, lse, n_frames, self.blank, pad_id=-1))
        return [dict(tokens=tok[b, :n[b]].copy(), start=start[b, :n[b]].copy(), length=length[b, :n[b]].copy(), logprob=lp[b, :n[b]].copy())
                for b in range(len(n))]

    @torch.inference_mode()
    def score(self, units, n_frames, labels):
        """labels: one id sequence per clip -> nll fp32 [B] on the device = F.ctc_loss(reduction='none') (HF's .loss with
        ctc_loss_reduction="sum" is its sum)"""
        pad, ll = self._labels(labels, units.shape[0] if units.dim() == 3 else 1)      # (a bad label is refused before anything is uploaded)
        units, n_frames = self._args(units, n_frames)
        return native.ctc_score(units, n_frames, self._wd, self._bd, self.blank, torch.from_numpy(pad).to(units.device), ll)

    @torch.inference_mode()
    def align(self, units, n_frames, labels):
        """-> one dict per clip: score (the Viterbi path's log-probability, -inf if the transcript does not fit), frame_label [n_frames]
        (index into the transcript, -1 on blanks), segments [L, 2] (first frame, one past the last) and logprob [L], on the host"""
        pad, ll = self._labels(labels, units.shape[0] if units.dim() == 3 else 1)      # (a bad label is refused before anything is uploaded)
        units, n_frames = self._args(units, n_frames)
        ps, fl, seg, llp = (t.cpu().numpy() for t in native.ctc_align(units, n_frames, self._wd, self._bd, self.blank, torch.from_numpy(pad).to(units.device), ll))
        nf = np.asarray(n_frames.cpu() if torch.is_tensor(n_frames) else n_frames).reshape(-1)
        return [dict(score=float(ps[b]), frame_label=fl[b, :int(nf[b])].copy(), segments=seg[b, :ll[b]].copy(), logprob=llp[b, :ll[b]].copy())
                for b in range(len(ll))]

    def decode(self, tokens):
        """ids -> text with the checkpoint's vocab.json ('|' is HF's word delimiter)"""
        if self.vocab is None:
            raise ValueError("CTCHead.decode needs a vocab (vocab.json next to the checkpoint, or vocab=)")
        return "".join(self.vocab[int(t)] for t in tokens).replace("|", " ")


def edit_distance(a, b):
    """plain Levenshtein distance between two sequences (tools/ctc_eval.py's error rate)"""
    a, b = list(a), list(b)
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[-1]
