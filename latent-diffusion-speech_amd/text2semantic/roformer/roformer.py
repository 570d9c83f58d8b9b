"""`Roformer` / `get_model` with the reference's names, constructor arguments, attributes, state_dict keys and `generate` signature
(reference text2semantic/roformer/roformer.py:8-255).  The reference drives HF transformers' RoFormerModel (phone/tone encoder) and
RoFormerForCausalLM (+ cross-attention) through GenerationMixin; here the encoder prefill, the key/value-cached decode loop and the
token choice run in liblds (csrc/lm.hip).  torch keeps the parameters and draws the sampling uniforms.

Scope: phone mode (the 'text' mode fetches a BERT tokenizer from the hub), inference only (`forward` = the gradient-carrying
teacher-forced training entry), right-padded batches; greedy decoding, sampling and greedy beam search (num_beams 2 .. 8), each with
optional n-gram blocking; greedy decoding and sampling may continue a given semantic prompt (`semantic_prompt`, one length per row);
`score`: teacher-forced log-probs, loss and ranks of given tokens in one causal pass (no gradients).
Not built: beam sampling, beam search from a prompt and the end gate (see `generate`)."""
from collections import namedtuple

import numpy as np
import torch
from torch import nn

from lds import arch, native
from lds.paramtree import ParamTree


def _get(cfg, key, default=None):
    """read a field from a dict, an HF config object or any namespace"""
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


# what `Roformer.score` returns: loss [] (HF's mean over the counted positions), token_logprobs [B,T-1] (0 where not counted), ranks int32
# [B,T-1] (-1 where not counted), seq_logprob [B], n_tokens int32 [] (counted positions), logits [B,T,V] or None
LMScore = namedtuple("LMScore", "loss token_logprobs ranks seq_logprob n_tokens logits")


def get_model(n_spk, **kwargs):
    return Roformer(
        encoder_config=dict(kwargs["model"]["encoder"], is_decoder=False),
        decoder_config=dict(kwargs["model"]["decoder"], is_decoder=True),
        mode=kwargs["model"]["mode"],
        semantic_kmeans_num=kwargs["model"]["semantic_kmeans_num"],
        codebook_path=kwargs["model"]["codebook_path"],
        n_spk=n_spk,
        use_flash_attn=kwargs["train"]["use_flash_attn"])


class Roformer(ParamTree):
    def __init__(self, encoder_config, decoder_config, mode="phone", semantic_kmeans_num=10000, codebook_path="pretrain/semantic_codebook.pt",
                 n_spk=1, use_flash_attn=False, **kwargs):
        if "text" in mode:
            raise NotImplementedError("mode 'text' needs BertTokenizer.from_pretrained (network); phone mode is built")
        if "phone" not in mode:
            raise ValueError(f"unknown mode {mode!r}")
        for k in ("hidden_size", "num_attention_heads", "intermediate_size"):
            if _get(encoder_config, k) != _get(decoder_config, k):
                raise NotImplementedError("encoder and decoder widths must match (reference configs/config.yaml:60-83)")
        if _get(encoder_config, "hidden_act", "gelu") != "gelu" or _get(decoder_config, "hidden_act", "gelu") != "gelu":
            raise NotImplementedError("only hidden_act 'gelu' is built")
        # one sinusoid table and one LayerNorm epsilon serve both stacks (lds_lm_cfg): configurations whose stacks differ are refused
        # rather than run with the encoder's values (HF RoFormerConfig defaults: 1536 positions, eps 1e-12)
        for k, dflt in (("max_position_embeddings", 1536), ("layer_norm_eps", 1e-12)):
            if _get(encoder_config, k, dflt) != _get(decoder_config, k, dflt):
                raise NotImplementedError(f"encoder and decoder must agree on {k}")
        cfg = arch.roformer_config(
            n_spk=n_spk, semantic_kmeans_num=semantic_kmeans_num, hidden_size=_get(encoder_config, "hidden_size"),
            num_attention_heads=_get(encoder_config, "num_attention_heads"), intermediate_size=_get(encoder_config, "intermediate_size"),
            encoder_layers=_get(encoder_config, "num_hidden_layers"), decoder_layers=_get(decoder_config, "num_hidden_layers"),
            max_position_embeddings=_get(encoder_config, "max_position_embeddings", 1536),
            layer_norm_eps=float(_get(encoder_config, "layer_norm_eps", 1e-12)))
        super().__init__(arch.roformer_param_shapes(cfg), seed=0)
        self.cfg = cfg
        self.mode, self.n_spk, self.use_flash_attn = mode, n_spk, use_flash_attn
        self.BOS, self.EOS, self.PAD = cfg["text_bos"], cfg["text_eos"], cfg["text_pad"]
        self.num_tones = arch.NUM_TONES
        self.semantic_bos_token_id, self.semantic_eos_token_id, self.semantic_pad_token_id = cfg["sem_bos"], cfg["sem_eos"], cfg["sem_pad"]
        with torch.no_grad():
            for k, v in arch.roformer_init_state(cfg, 0).items():
                self._leaf(k).copy_(torch.from_numpy(v))
        # weight tying like RoFormerForCausalLM: the LM head shares the decoder's word embeddings and the output-only bias
        pred = self.semantic_decoder.cls.predictions
        pred.decoder.weight = self.semantic_decoder.roformer.embeddings.word_embeddings.weight
        pred.decoder.bias = pred.bias
        try:      # reference roformer.py:110-115: seed the token embeddings with the k-means centres when the widths agree
            from cluster import get_cluster_model
            self.quantizer = get_cluster_model(codebook_path)
            centers = self.quantizer.cluster_centers_
            if self.semantic_decoder.roformer.embeddings.word_embeddings.weight.shape[1] == centers.shape[1]:
                self.semantic_decoder.roformer.embeddings.word_embeddings.weight.data[:semantic_kmeans_num] = torch.from_numpy(centers.copy())
        except Exception:
            pass
        self.spk_emb_enabled = n_spk is not None and n_spk > 1
        self._native = None

    def _leaf(self, key):
        node = self
        parts = key.split(".")
        for p in parts[:-1]:
            node = node._modules[p]
        return node._parameters[parts[-1]]

    # parameter changes drop the packed copy (see UNet1DConditionModel)
    def _apply(self, fn, *a, **k):
        self._native = None
        return super()._apply(fn, *a, **k)

    def _load_from_state_dict(self, *a, **k):
        self._native = None
        return super()._load_from_state_dict(*a, **k)

    def native(self):
        if self._native is None:
            self._native = native.LM(self.cfg, dict(self.state_dict()))
        return self._native

    def forward(self, *a, **k):
        raise NotImplementedError("teacher-forced training forward (with gradients) is out of scope for the MI355X inference build; "
                                  "Roformer.score gives the teacher-forced loss, log-probs and ranks without gradients")

    @staticmethod
    def _mask_to_lengths(attention_mask):
        """HF padding mask [B,L] (1 = real, 0 = pad) of a RIGHT-padded batch -> int32 [B] real lengths (what the kernels take)"""
        if attention_mask is None:
            return None
        m = attention_mask.to(torch.int64)
        n = m.sum(-1)
        L = m.shape[-1]
        if not bool(((torch.arange(L, device=m.device)[None] < n[:, None]).to(torch.int64) == m).all()) or bool((n < 1).any()):
            raise NotImplementedError("only right-padded batches are built: every attention_mask row must be ones followed by zeros")
        return n.to(torch.int32).contiguous()

    def _check_prompt(self, B, semantic_prompt, prompt_attention_mask, max_length, num_beams):
        """the checks of `generate`'s decoder prompt (no device work beyond reading the prompt itself) -> the rows' lengths as a list of ints"""
        if num_beams > 1:
            # the beams' key/value ancestry tables start at BOS: a prefix would have to be replicated per beam first
            raise NotImplementedError("beam search from a prompt (num_beams > 1 with semantic_prompt) is not built")
        if semantic_prompt.dim() != 2 or semantic_prompt.shape[0] != B or semantic_prompt.shape[1] < 1:
            raise ValueError(f"semantic_prompt must be [B, P] with B = {B} and P >= 1, got {tuple(semantic_prompt.shape)}")
        if B > 64:
            raise ValueError(f"a prompted decode takes at most 64 rows, got {B}")
        P = int(semantic_prompt.shape[1])
        if prompt_attention_mask is not None and tuple(prompt_attention_mask.shape) != (B, P):
            raise ValueError(f"prompt_attention_mask must have semantic_prompt's shape {(B, P)}, got {tuple(prompt_attention_mask.shape)}")
        n = self._mask_to_lengths(prompt_attention_mask)
        lens = [P] * B if n is None else [int(v) for v in n.tolist()]
        sp = semantic_prompt.detach().to("cpu", torch.int64)
        for b, pl in enumerate(lens):
            if pl >= max_length:      # HF raises ValueError as well: max_length counts the prompt
                raise ValueError(f"row {b}: the prompt has {pl} tokens, which leaves no room below max_length = {max_length} (the total length)")
            if int(sp[b, 0]) != self.semantic_bos_token_id:
                raise ValueError(f"row {b}: semantic_prompt must start with BOS ({self.semantic_bos_token_id}), got {int(sp[b, 0])}")
            body = sp[b, 1:pl]
            if bool(((body < 0) | (body >= self.cfg["semantic_kmeans_num"])).any()):
                raise ValueError(f"row {b}: prompt ids after BOS and inside the length must lie in [0, {self.cfg['semantic_kmeans_num']})")
        return lens

    @torch.no_grad()
    def encode(self, phone, tone, spk_id=None, attention_mask=None):
        """encoder_hidden_states [B,L,hidden] of reference roformer.py:196-214 (rows of padded positions are computed but never read)"""
        return self.native().encode(phone, tone, spk_id if self.spk_emb_enabled else None, self._mask_to_lengths(attention_mask))

    @torch.no_grad()
    def generate(self, phone, tone, attention_mask=None, use_cache=None, max_length=1024, do_sample=True, temperature=1.0, top_k=5, top_p=0.8,
                 repetition_penalty=1.2, num_beams=1, no_repeat_ngram_size=0, early_stopping=True, spk_id=None, end_gate_threshold=None,
                 return_logits=False, semantic_prompt=None, prompt_attention_mask=None, uniforms=None, **kwargs):
        """The reference's `generate` (roformer.py:179-244), plus the decoder prompt its HF call accepts as input_ids= (roformer.py:235-242):
        semantic_prompt [B,P] int64, BOS first like `score`'s `semantic`, right-padded with prompt_attention_mask [B,P] (ones then zeros) when the
        rows' prompts differ in length.  Every row continues its own prompt exactly as it would alone; max_length is the total length, prompt
        included (HF); the returned rows start with the prompt; the repetition penalty and the n-gram ban see the prompt as history.
        uniforms [max_length - 1, B] (sampling): row b's s-th generated token uses uniforms[s][b]; None draws them with torch.rand as always.
        With return_logits, logits[s][b] are the logits that chose row b's s-th generated token."""
        if end_gate_threshold is not None:
            # reference roformer.py:49-57 sets the WHOLE score row to +inf once softmax(scores)[eos] passes the threshold: greedy then picks
            # token 0 and sampling makes torch.multinomial raise on NaN probabilities -- there is no coherent behaviour to restate
            raise NotImplementedError("the end gate is not built: the reference's EndGateLogitsProcessor sets the whole score row to +inf, "
                                      "after which greedy picks token 0 and sampling raises")
        if isinstance(num_beams, bool) or not isinstance(num_beams, (int, np.integer)) or not 1 <= num_beams <= 8:
            raise ValueError(f"num_beams must be an integer in 1 .. 8, got {num_beams!r}")
        if isinstance(no_repeat_ngram_size, bool) or not isinstance(no_repeat_ngram_size, (int, np.integer)) or no_repeat_ngram_size < 0:
            raise ValueError(f"no_repeat_ngram_size must be an integer >= 0, got {no_repeat_ngram_size!r}")
        num_beams, no_repeat_ngram_size = int(num_beams), int(no_repeat_ngram_size)
        if num_beams > 1 and do_sample:
            # HF draws 2 * num_beams candidates without replacement through torch.multinomial; the inverse-CDF draw over recorded uniforms
            # that stands in for the single-sample draw has no agreed form for more than one sample
            raise NotImplementedError("beam sampling (num_beams > 1 with do_sample=True) is not built; pass do_sample=False for greedy beam search")
        if num_beams > 1 and return_logits:
            raise NotImplementedError("return_logits is not available with num_beams > 1")
        if num_beams > 1 and early_stopping not in (True, False, "never"):
            raise ValueError(f"early_stopping must be True, False or 'never', got {early_stopping!r}")
        # top_k as HF's TopKLogitsWarper: None / 0 = no filter (the draw runs over the whole vocabulary), k keeps the k largest scores and every
        # score tied with the k-th (22_infer_tts.py:83-98 passes top_k = 5); more than 64 survivors are not built
        top_k = 0 if top_k is None else int(top_k)
        if do_sample and not (0 <= top_k <= 64):
            raise NotImplementedError("sampling is built for top_k = None / 0 (no filter) or 1 <= top_k <= 64")
        enc_len = self._mask_to_lengths(attention_mask)      # reference roformer.py:209-236: the encoder's mask and the cross-attention's
        prompt_len = None
        if semantic_prompt is None and prompt_attention_mask is not None:
            raise ValueError("prompt_attention_mask needs semantic_prompt")
        if semantic_prompt is not None:      # everything about the prompt is checked before any device work
            prompt_len = self._check_prompt(phone.shape[0], semantic_prompt, prompt_attention_mask, max_length, num_beams)
        if not phone.is_cuda:
            raise RuntimeError("Roformer.generate needs tensors on a HIP device (no CPU fallback)")
        enc = self.native().encode(phone, tone, spk_id if self.spk_emb_enabled else None, enc_len)
        B = enc.shape[0]
        if not do_sample:
            uniforms = None
        elif uniforms is None:
            uniforms = torch.rand(max_length - 1, B, device=enc.device)      # one draw per step and sequence
        else:
            uniforms = uniforms.to(device=enc.device, dtype=torch.float32)
            if uniforms.dim() != 2 or uniforms.shape[1] != B or uniforms.shape[0] < max_length - (min(prompt_len) if prompt_len else 1):
                raise ValueError(f"uniforms must be [steps, B = {B}] with one row per generated position, got {tuple(uniforms.shape)}")
            if uniforms.shape[0] < max_length - 1:      # the library's layout is [max_length - 1, B]; the rows past the last step are never read
                uniforms = torch.cat([uniforms, uniforms.new_zeros(max_length - 1 - uniforms.shape[0], B)])
        if prompt_len is not None:
            P = max(prompt_len)
            prompt = semantic_prompt[:, :P].to(device=enc.device, dtype=torch.int64)
            toks, logits = self.native().generate_prompt(enc, prompt, prompt_len, max_length, do_sample, top_k, top_p, temperature, repetition_penalty,
                                                         uniforms, return_logits, enc_len, no_repeat_ngram_size=no_repeat_ngram_size)
            return (toks, logits) if return_logits else toks
        # beams: enc and enc_len stay one row per item; the library maps beam row r to item r // num_beams
        toks, logits = self.native().generate(enc, max_length, do_sample, top_k, top_p, temperature, repetition_penalty, uniforms, return_logits, enc_len,
                                              num_beams=num_beams, no_repeat_ngram_size=no_repeat_ngram_size, early_stopping=early_stopping)
        return (toks, logits) if return_logits else toks

    @torch.no_grad()
    def score(self, phone, tone, semantic, attention_mask=None, encoder_attention_mask=None, labels=None, spk_id=None, return_logits=False):
        """Teacher-forced scoring of `semantic` [B,T] (BOS first, as the reference's loader builds it) under the LM, all positions in one
        causal pass.  The arguments are those of the reference's `forward` (roformer.py:138-176; `labels` defaults to `semantic` as in
        dataloader.py:181-182); the logits at position t are those of the PREFIX semantic[:, :t + 1] -- what `generate` computes at step t,
        bit for bit -- not those of the reference's one-call forward, which is non-causal on transformers 5.x.
        Position t (0 <= t <= len_b - 2) is counted when labels[b, t + 1] != -100 (HF's shift); ids at and beyond a row's length have no
        effect on any counted output.  Returns an LMScore."""
        if semantic.dim() != 2 or semantic.shape[0] != phone.shape[0]:
            raise ValueError(f"semantic must be [B, T] with B = {phone.shape[0]}, got {tuple(semantic.shape)}")
        B, T = semantic.shape
        if T < 2 or T > self.cfg["max_pos"]:
            raise ValueError(f"semantic needs 2 <= T <= max_position_embeddings = {self.cfg['max_pos']}, got T = {T}")
        if labels is not None and tuple(labels.shape) != (B, T):
            raise ValueError(f"labels must have semantic's shape {(B, T)}, got {tuple(labels.shape)}")
        if attention_mask is not None and tuple(attention_mask.shape) != (B, T):
            raise ValueError(f"attention_mask must have semantic's shape {(B, T)}, got {tuple(attention_mask.shape)}")
        enc_len, sem_len = self._mask_to_lengths(encoder_attention_mask), self._mask_to_lengths(attention_mask)
        if not (phone.is_cuda and tone.is_cuda and semantic.is_cuda):
            raise RuntimeError("Roformer.score needs tensors on a HIP device (no CPU fallback)")
        semantic = semantic.to(torch.int64)
        labels = labels.to(device=semantic.device, dtype=torch.int64) if labels is not None else None
        # the library clamps ids on the way into the embedding: what it would hide is refused here (ids inside the lengths; labels may be -100)
        V = self.cfg["sem_vocab"]
        inside = torch.ones_like(semantic, dtype=torch.bool) if sem_len is None else torch.arange(T, device=semantic.device)[None] < sem_len[:, None]
        if bool((inside & ((semantic < 0) | (semantic >= V))).any()):
            raise ValueError(f"semantic ids inside the sequence lengths must lie in [0, {V})")
        if labels is not None and bool((inside & (labels != -100) & ((labels < 0) | (labels >= V))).any()):
            raise ValueError(f"labels inside the sequence lengths must be -100 or lie in [0, {V})")
        enc = self.native().encode(phone, tone, spk_id if self.spk_emb_enabled else None, enc_len)
        lp, ranks, loss, n, logits = self.native().score(enc, semantic, sem_len, labels, enc_len, return_logits)
        return LMScore(loss, lp, ranks, lp.double().sum(-1).float(), n, logits)
