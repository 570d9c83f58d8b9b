"""Whisper's audio encoder as parameter holders over the native handle (reference encoder/whisper/model.py:10-137).  The modules carry
the reference's `state_dict` keys, so a reference checkpoint's `model_state_dict` loads unchanged; `AudioEncoder.forward(mel)` runs
lds_whisper_encode_mel.  The reference's `Whisper(dims)` builds no decoder, and neither does this one by default; `Whisper(dims,
decoder=True)` adds OpenAI's `TextDecoder` over lds_whisper_decoder_* (greedy speech to text: `logits`, `forward`, `decode`, `score`,
`detect_language`).  Not built (NotImplementedError): sampling and temperature fallback, beam search, timestamp decoding, word alignment
from `alignment_heads`, long-form windows, fp16."""
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


class TextDecoder(nn.Module):
    """OpenAI's TextDecoder as a parameter holder (its `state_dict` keys: token_embedding.weight, positional_embedding, blocks.N.*, ln.*);
    `forward(x, xa)` runs lds_whisper_decoder_cross + lds_whisper_decoder_logits."""

    def __init__(self, n_vocab: int, n_ctx: int, n_state: int, n_head: int, n_layer: int, n_audio_ctx: int = 1500):
        super().__init__()
        for k, s in arch.whisper_decoder_param_shapes(n_vocab, n_ctx, n_state, n_layer).items():
            AudioEncoder._register(self, k[len("decoder."):], torch.zeros(s))
        self.n_vocab, self.n_ctx, self.n_state, self.n_head, self.n_layer, self.n_audio_ctx = n_vocab, n_ctx, n_state, n_head, n_layer, n_audio_ctx
        self._native = None

    def _load_from_state_dict(self, *a, **k):
        self._native = None
        return super()._load_from_state_dict(*a, **k)

    def native(self):
        if self._native is None:
            state = {"decoder." + k: v.detach().cpu() for k, v in self.state_dict().items()}
            self._native = native.WhisperDecoder(self.n_vocab, self.n_ctx, self.n_state, self.n_head, self.n_layer, self.n_audio_ctx, state)
        return self._native

    def cross(self, xa, n_frames=None):
        """the cross keys / values of a batch of encoder outputs [B, T, n_state]; the calls that follow read them"""
        if not xa.is_cuda:
            raise RuntimeError("TextDecoder needs the audio features on a HIP device (no CPU fallback)")
        if xa.dtype != torch.float32:
            raise NotImplementedError("the native decoder is fp32 only")
        self.native().cross(xa, n_frames)

    @torch.no_grad()
    def forward(self, x, xa, n_frames=None):
        """x int64 [B, S] tokens, xa [B, T, n_state] audio features on a HIP device -> logits [B, S, n_vocab]"""
        self.cross(xa, n_frames)
        return self.native().logits(x.to(torch.int64))


class Whisper(nn.Module):
    def __init__(self, dims: ModelDimensions, decoder: bool = False):
        """decoder=False (the default) is the reference's Whisper(dims): the audio encoder alone, the same `state_dict`."""
        super().__init__()
        self.dims = dims
        self.encoder = AudioEncoder(dims.n_mels, dims.n_audio_state, dims.n_audio_head, dims.n_audio_layer, dims.n_audio_ctx)
        if decoder:
            self.decoder = TextDecoder(dims.n_vocab, dims.n_text_ctx, dims.n_text_state, dims.n_text_head, dims.n_text_layer, dims.n_audio_ctx)

    def load_state_dict(self, state_dict, *a, **k):
        self.encoder._native = None
        if hasattr(self, "decoder"):
            self.decoder._native = None
        return super().load_state_dict(state_dict, *a, **k)

    def _dec(self):
        if not hasattr(self, "decoder"):
            raise RuntimeError("this Whisper was built without its text decoder: Whisper(dims, decoder=True)")
        return self.decoder

    def logits(self, tokens, audio_features):
        return self._dec()(tokens, audio_features)

    def forward(self, mel, tokens):
        return self._dec()(tokens, self.encoder(mel))

    @property
    def is_multilingual(self):
        return self.dims.n_vocab >= 51865

    @property
    def num_languages(self):
        return self.dims.n_vocab - 51765 - int(self.is_multilingual)

    def special_tokens(self, **override):
        return arch.whisper_special_tokens(self.dims.n_vocab, **override)

    @torch.no_grad()
    def decode(self, audio_features, n_frames=None, prompt=None, max_new_tokens=224, suppress_tokens=None, begin_suppress_tokens=None,
               eot=None, language="en", task="transcribe", temperature=0.0, beam_size=None, without_timestamps=True, return_logits=False):
        """Greedy decode of a batch of encoder outputs [B, T, n_state] (n_frames: every clip's own frame count).  prompt: None (the
        `<|startoftranscript|><|language|><|task|><|notimestamps|>` sequence of the special-token table for every row), an int64 [B, P]
        tensor, or a list of B id lists (each row its own length: a `<|startofprev|>` prefix).  suppress_tokens None: every special token
        but <|endoftext|> (what a text-only transcript may not hold); begin_suppress_tokens None: <|endoftext|>.
        Returns (tokens [B, n] with the prompt in front, EOS kept, PAD = eot after it; token_logprob [B, max_new_tokens]; avg_logprob [B] =
        the sum over the generated ids, EOS included, divided by their number), plus the raw logits [steps, B, n_vocab] if return_logits."""
        if temperature != 0.0:
            raise NotImplementedError("sampling and temperature fallback are not built: temperature must be 0")
        if beam_size not in (None, 1):
            raise NotImplementedError("beam search is not built")
        if not without_timestamps:
            raise NotImplementedError("timestamp decoding (ApplyTimestampRules) is not built")
        dec = self._dec()
        B = int(audio_features.shape[0])
        dev = audio_features.device
        need_table = prompt is None or suppress_tokens is None or begin_suppress_tokens is None or eot is None
        sp = self.special_tokens() if need_table else None
        eot = sp["eot"] if eot is None else int(eot)
        if prompt is None:
            if language not in sp["languages"]:
                raise ValueError(f"unknown language {language!r}")
            if task not in ("transcribe", "translate"):
                raise ValueError(f"task must be transcribe or translate, got {task!r}")
            prompt = [[sp["sot"], sp["languages"][language], sp[task], sp["notimestamps"]]] * B
        if isinstance(prompt, torch.Tensor):
            plen = [int(prompt.shape[1])] * B
            ids = prompt.to(device=dev, dtype=torch.int64)
        else:
            plen = [len(r) for r in prompt]
            ids = torch.full((B, max(plen)), eot, dtype=torch.int64)
            for b, r in enumerate(prompt):
                ids[b, : len(r)] = torch.as_tensor(list(r), dtype=torch.int64)
            ids = ids.to(dev)
        if suppress_tokens is None:
            suppress_tokens = [i for i in range(sp["sot"], self.dims.n_vocab)]
        if begin_suppress_tokens is None:
            begin_suppress_tokens = [eot]
        dec.cross(audio_features, n_frames)
        toks, tlp, slp, lg = dec.native().generate(ids, plen, max_new_tokens, eot, eot, suppress_tokens, begin_suppress_tokens, return_logits)
        cap = min(max(plen) + int(max_new_tokens), self.dims.n_text_ctx)
        cnt = []
        for b in range(B):      # generated ids up to and including the first EOS inside the row's own budget
            row = toks[b, plen[b]: plen[b] + min(int(max_new_tokens), cap - plen[b])]
            stop = (row == eot).nonzero()
            cnt.append(int(stop[0]) + 1 if stop.numel() else int(row.numel()))
        avg = slp / torch.as_tensor(cnt, dtype=torch.float32, device=dev).clamp(min=1)
        return (toks, tlp, avg, lg) if return_logits else (toks, tlp, avg)

    @torch.no_grad()
    def score(self, audio_features, tokens, tok_len=None, n_frames=None, labels=None, return_logits=False):
        """Teacher-forced scoring of transcripts: tokens int64 [B, S] (prompt and text), tok_len int32 [B] or None.  Returns lds_lm_score's
        (logprobs [B, S-1], ranks [B, S-1], loss, n_counted, logits or None) without storing B * S * n_vocab logits unless asked."""
        dec = self._dec()
        dec.cross(audio_features, n_frames)
        dev = audio_features.device
        tl = None if tok_len is None else torch.as_tensor(tok_len, dtype=torch.int32).to(dev)
        return dec.native().logits(tokens.to(device=dev, dtype=torch.int64), tl, labels, return_logits=return_logits, score=True)

    @torch.no_grad()
    def detect_language(self, audio_features, n_frames=None):
        """One decoder step from <|startoftranscript|>, then a softmax over the language-token columns (openai-whisper's
        detect_language).  Returns (language ids [B], probabilities [B, num_languages] in the table's order)."""
        sp = self.special_tokens()
        B = int(audio_features.shape[0])
        dev = audio_features.device
        # (the entry takes S >= 2: the second position's row is computed and dropped; the first does not see it)
        x = torch.tensor([[sp["sot"], sp["sot"]]] * B, dtype=torch.int64, device=dev)
        self._dec().cross(audio_features, n_frames)
        lg = self.decoder.native().logits(x)[:, 0]
        lang_ids = torch.as_tensor(list(sp["languages"].values()), device=dev)
        probs = torch.softmax(lg[:, lang_ids], dim=-1)
        return lang_ids[probs.argmax(-1)], probs

    def embed_audio(self, mel):
        return self.encoder(mel)

    @property
    def device(self):
        return next(self.parameters()).device
