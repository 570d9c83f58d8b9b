"""`Llama` with the reference's name, constructor arguments, attributes, state_dict keys and `generate` signature (reference
text2semantic/llama/llama.py:23-184).  The reference drives HF transformers' LlamaForCausalLM through GenerationMixin over one token stream
[phone BOS, phones, phone EOS, semantic BOS, semantic tokens ...]; here the causal prefill of that prompt, the key/value-cached decode loop and
the token choice run in liblds (csrc/llama.hip; the choice kernels are csrc/lm.hip's).  torch keeps the parameters and draws the sampling
uniforms.  transformers is not imported: `config` is read field by field from a dict, an HF LlamaConfig or any namespace.

The numbering is the reference's (llama.py:36-61): phone ids 0 .. 107, phone BOS / EOS / PAD 108 / 109 / 110, semantic token t at id 108 + t,
semantic BOS / EOS / PAD at 108 + K, + 1, + 2 -- so the phone BOS, EOS and PAD ids coincide with the shifted semantic ids 0, 1, 2.  `generate`
bans every id below 108 (llama.py:170), returns the generated ids minus 108 with EOS (K + 1) kept (llama.py:182), and hands the WHOLE stream
to HF's processors: with a repetition penalty the semantic tokens 0 and 1 are penalised from the first step on (ids 108 and 109 are in every
prompt), and the prompt's n-grams count for the n-gram ban.

Scope: phone mode, inference, num_beams 1 (greedy and sampling, each with the repetition penalty and n-gram blocking), each optionally
continuing a semantic prompt (`semantic_prompt`, one length per row); `score` / `score_ids`: teacher-forced log-probs, loss and ranks over
the whole vocabulary in one causal pass (the reference `forward`'s numbers, no gradients).
Not built (each raises): mode 'text', the end gate, beam search, `forward` (training), attention_bias / mlp_bias, a rope type other than
default, hidden_act other than silu."""
import numpy as np
import torch

from lds import arch, native
from lds.paramtree import ParamTree
from text2semantic.roformer.roformer import LMScore, _get


def get_model(n_spk, **kwargs):
    """The factory `get_language_model` calls for model.type == "llama".  The reference has none (its utils.py knows "roformer" only and its
    Llama is built by hand, llama.py:186-193): model.llama holds LlamaConfig's fields, next to the keys the RoFormer's section has as well."""
    m = kwargs["model"]
    return Llama(config=dict(m["llama"]), mode=m.get("mode", "phone"), semantic_kmeans_num=m["semantic_kmeans_num"],
                 codebook_path=m.get("codebook_path", "pretrain/semantic_codebook.pt"), use_flash_attn=kwargs.get("train", {}).get("use_flash_attn", False))


class _Config:
    """the fields of the caller's config that the model reads, plus the ids the reference's constructor writes into it (llama.py:56-61)"""


class Llama(ParamTree):
    def __init__(self, config, mode="phone", semantic_kmeans_num=10000, codebook_path="pretrain/semantic_codebook.pt", use_flash_attn=False):
        if "text" in mode:
            raise NotImplementedError("mode 'text' needs BertTokenizer.from_pretrained (network); phone mode is built")
        if "phone" not in mode:
            raise ValueError(f"unknown mode {mode!r}")
        if _get(config, "attention_bias", False) or _get(config, "mlp_bias", False):
            raise NotImplementedError("attention_bias / mlp_bias are not built: the projections are bias-free (LlamaConfig's default)")
        if _get(config, "hidden_act", "silu") != "silu":
            raise NotImplementedError("only hidden_act 'silu' is built")
        rope = _get(config, "rope_parameters", None) or _get(config, "rope_scaling", None) or {}
        rope_type = _get(rope, "rope_type", _get(rope, "type", "default"))
        if rope_type != "default":
            raise NotImplementedError(f"rope type {rope_type!r} is not built: only the default rotary embedding")
        theta = _get(rope, "rope_theta", None) or _get(config, "rope_theta", None) or 10000.0
        heads = _get(config, "num_attention_heads", 32)
        cfg = arch.llama_config(
            semantic_kmeans_num=semantic_kmeans_num, hidden_size=_get(config, "hidden_size", 4096), num_attention_heads=heads,
            num_key_value_heads=_get(config, "num_key_value_heads", None) or heads, head_dim=_get(config, "head_dim", None),
            intermediate_size=_get(config, "intermediate_size", 11008), num_hidden_layers=_get(config, "num_hidden_layers", 32),
            max_position_embeddings=_get(config, "max_position_embeddings", 2048), rms_norm_eps=float(_get(config, "rms_norm_eps", 1e-6)),
            rope_theta=float(theta))
        if cfg["heads"] % cfg["kv_heads"]:
            raise ValueError(f"num_key_value_heads {cfg['kv_heads']} must divide num_attention_heads {cfg['heads']}")
        super().__init__(arch.llama_param_shapes(cfg), seed=0)
        self.cfg = cfg
        self.mode, self.use_flash_attn = mode, use_flash_attn
        self.BOS, self.EOS, self.PAD = cfg["text_bos"], cfg["text_eos"], cfg["text_pad"]
        self.num_tones = arch.NUM_TONES
        self.semantic_token_shift = cfg["shift"]
        # the reference writes the ids into the caller's config object (llama.py:56-61); a dict gets them as keys, anything else as attributes
        for k, v in (("bos_token_id", cfg["bos"]), ("eos_token_id", cfg["eos"]), ("pad_token_id", cfg["pad"]), ("vocab_size", cfg["vocab"])):
            if isinstance(config, dict):
                config[k] = v
            else:
                setattr(config, k, v)
        if isinstance(config, dict):
            ns = _Config()
            ns.__dict__.update(config)
            config = ns
        self.config = config
        with torch.no_grad():
            for k, v in arch.llama_init_state(cfg, 0).items():
                self._leaf(k).copy_(torch.from_numpy(v))
        try:      # reference llama.py:66-71: seed the token embeddings with the k-means centres when the widths agree -- rows len(symbols) - 1 ..,
            # one row below the first semantic id, as the reference has it
            from cluster import get_cluster_model
            self.quantizer = get_cluster_model(codebook_path)
            centers = self.quantizer.cluster_centers_
            emb = self.llama.model.embed_tokens.weight
            if emb.shape[1] == centers.shape[1]:
                emb.data[arch.PHONE_SYMBOLS - 1:arch.PHONE_SYMBOLS + semantic_kmeans_num - 1] = torch.from_numpy(centers.copy())
        except Exception:
            pass
        # HF LlamaRotaryEmbedding's inverse frequencies, by its own expression in torch (its vectorised fp32 pow is not correctly rounded, and
        # one ulp here is 6e-5 rad at position 1000): not a parameter, handed to the library next to the weights
        d = cfg["head_dim"]
        self.inv_freq = 1.0 / (cfg["rope_theta"] ** (torch.arange(0, d, 2, dtype=torch.int64).to(dtype=torch.float) / d))
        self._native = None

    def _leaf(self, key):
        node = self
        parts = key.split(".")
        for p in parts[:-1]:
            node = node._modules[p]
        return node._parameters[parts[-1]]

    # parameter changes drop the packed copy (see Roformer)
    def _apply(self, fn, *a, **k):
        self._native = None
        return super()._apply(fn, *a, **k)

    def _load_from_state_dict(self, *a, **k):
        self._native = None
        return super()._load_from_state_dict(*a, **k)

    def native(self):
        if self._native is None:
            state = dict(self.state_dict())
            state["llama.model.rotary_emb.inv_freq"] = self.inv_freq
            self._native = native.Llama(self.cfg, state)
        return self._native

    def forward(self, *a, **k):
        raise NotImplementedError("teacher-forced training forward (with gradients) is out of scope for the MI355X inference build")

    def input_ids(self, phone, attention_mask=None):
        """llama.py:147-152 for every row of a right-padded batch: row b = [BOS, phones_b, EOS, semantic BOS], padded with the config's pad id
        -> (input_ids [B, L + 3] int64 on phone's device, the rows' lengths as a list of ints)"""
        if phone.dim() != 2 or phone.shape[1] < 1:
            raise ValueError(f"phone must be [B, L] with L >= 1, got {tuple(phone.shape)}")
        B, L = phone.shape
        if attention_mask is None:
            lens = [L] * B
        else:
            if tuple(attention_mask.shape) != (B, L):
                raise ValueError(f"attention_mask must have phone's shape {(B, L)}, got {tuple(attention_mask.shape)}")
            m = attention_mask.to(torch.int64)
            n = m.sum(-1)
            if not bool(((torch.arange(L, device=m.device)[None] < n[:, None]).to(torch.int64) == m).all()) or bool((n < 1).any()):
                raise NotImplementedError("only right-padded batches are built: every attention_mask row must be ones followed by zeros")
            lens = [int(v) for v in n.tolist()]
        ids = torch.full((B, L + 3), self.cfg["pad"], dtype=torch.int64, device=phone.device)
        ids[:, 0] = self.BOS
        ids[:, 1:L + 1] = phone.to(torch.int64)
        for b, n in enumerate(lens):
            ids[b, n + 1] = self.EOS
            ids[b, n + 2] = self.cfg["bos"]
            ids[b, n + 3:] = self.cfg["pad"]
        return ids, [n + 3 for n in lens]

    @staticmethod
    def _mask_to_lengths(mask, shape, name):
        """a right-padded HF mask [B, N] (ones then zeros; rows of zeros allowed) -> the rows' lengths as a list of ints; None = N everywhere"""
        if mask is None:
            return [int(shape[1])] * int(shape[0])
        if tuple(mask.shape) != tuple(shape):
            raise ValueError(f"{name} must have the shape {tuple(shape)}, got {tuple(mask.shape)}")
        m = mask.to(torch.int64)
        n = m.sum(-1)
        if not bool(((torch.arange(m.shape[1], device=m.device)[None] < n[:, None]).to(torch.int64) == m).all()):
            raise NotImplementedError(f"only right-padded batches are built: every {name} row must be ones followed by zeros")
        return [int(v) for v in n.tolist()]

    def _streams(self, phone, attention_mask, tails):
        """rows [108, phones_b, 109, tails[b] ...] (tails: one 1-D int64 tensor of model ids per row), right-padded with the config's pad id
        -> (ids [B, S] int64 on phone's device, the rows' lengths, the rows' phone counts)"""
        head, hl = self.input_ids(phone, attention_mask)
        nph = [n - 3 for n in hl]
        lens = [n + 2 + int(t.numel()) for n, t in zip(nph, tails)]
        ids = torch.full((len(lens), max(lens)), self.cfg["pad"], dtype=torch.int64, device=phone.device)
        for b, (n, t) in enumerate(zip(nph, tails)):
            ids[b, :n + 2] = head[b, :n + 2]
            ids[b, n + 2:lens[b]] = t.to(device=phone.device, dtype=torch.int64)
        return ids, lens, nph

    def _check_prompt(self, B, semantic_prompt, prompt_attention_mask):
        """the checks of `generate`'s semantic prompt -> one 1-D tensor of SHIFTED (model) ids per row, the semantic BOS first"""
        K = self.cfg["semantic_kmeans_num"]
        if semantic_prompt.dim() != 2 or semantic_prompt.shape[0] != B or semantic_prompt.shape[1] < 1:
            raise ValueError(f"semantic_prompt must be [B, P] with B = {B} and P >= 1, got {tuple(semantic_prompt.shape)}")
        lens = self._mask_to_lengths(prompt_attention_mask, semantic_prompt.shape, "prompt_attention_mask")
        sp = semantic_prompt.detach().to("cpu", torch.int64)
        tails = []
        for b, pl in enumerate(lens):
            if pl < 1 or int(sp[b, 0]) != K:
                raise ValueError(f"row {b}: semantic_prompt must start with the semantic BOS ({K})" + (f", got {int(sp[b, 0])}" if pl >= 1 else ""))
            body = sp[b, :pl]
            if bool(((body < 0) | (body > K + 2)).any()):
                raise ValueError(f"row {b}: prompt ids inside the length must lie in 0 .. {K + 2}")
            tails.append(body + self.semantic_token_shift)
        return tails

    @torch.no_grad()
    def score_ids(self, input_ids, attention_mask=None, labels=None, return_logits=False):
        """The `input_ids=` path of the reference's `forward` (llama.py:73-117, 103-114) without gradients: input_ids [B, S] of the model's
        vocabulary, right-padded with attention_mask [B, S] (ones then zeros); labels [B, S] default to input_ids (dataloader.py:182-183), -100
        is HF's ignore index.  One causal pass; position t of row b is counted when t + 1 lies inside the row and labels[b, t + 1] != -100
        (HF's shift); log-probabilities and ranks are taken over the whole vocabulary, phone ids included, as HF's loss does.  Returns an
        LMScore: loss [], token_logprobs [B, S - 1] (0 where not counted), ranks int32 [B, S - 1] (-1 where not counted), seq_logprob [B],
        n_tokens int32 [], logits [B, S, vocab] or None."""
        if input_ids.dim() != 2:
            raise ValueError(f"input_ids must be [B, S], got {tuple(input_ids.shape)}")
        B, S = input_ids.shape
        if S < 2 or S > self.cfg["max_pos"]:
            raise ValueError(f"input_ids needs 2 <= S <= max_position_embeddings = {self.cfg['max_pos']}, got S = {S}")
        if labels is not None and tuple(labels.shape) != (B, S):
            raise ValueError(f"labels must have input_ids' shape {(B, S)}, got {tuple(labels.shape)}")
        lens = None if attention_mask is None else self._mask_to_lengths(attention_mask, (B, S), "attention_mask")
        ids = input_ids.to(torch.int64)
        labels = labels.to(device=ids.device, dtype=torch.int64) if labels is not None else None
        ids_len = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=ids.device)
        # the library clamps ids on the way into the embedding: what it would hide is refused here (ids inside the lengths; labels may be -100)
        V = self.cfg["vocab"]
        inside = torch.ones_like(ids, dtype=torch.bool) if ids_len is None else torch.arange(S, device=ids.device)[None] < ids_len[:, None]
        if bool((inside & ((ids < 0) | (ids >= V))).any()):
            raise ValueError(f"input_ids inside the sequence lengths must lie in [0, {V})")
        if labels is not None and bool((inside & (labels != -100) & ((labels < 0) | (labels >= V))).any()):
            raise ValueError(f"labels inside the sequence lengths must be -100 or lie in [0, {V})")
        if not input_ids.is_cuda:
            raise RuntimeError("Llama.score_ids needs tensors on a HIP device (no CPU fallback)")
        lp, ranks, loss, n, logits = self.native().score(ids, ids_len, labels, return_logits)
        return LMScore(loss, lp, ranks, lp.double().sum(-1).float(), n, logits)

    def semantic_lengths(self, semantic, semantic_attention_mask=None):
        """the rows' token counts of `semantic` [B, T] in the numbering `generate` returns: a row ends behind its first K + 1 (EOS, kept) or
        before its first K + 2 (pad), whichever comes first; a semantic_attention_mask (ones then zeros) decides instead"""
        if semantic_attention_mask is not None:
            return self._mask_to_lengths(semantic_attention_mask, semantic.shape, "semantic_attention_mask")
        K = self.cfg["semantic_kmeans_num"]
        out = []
        for row in semantic.detach().to("cpu", torch.int64).tolist():
            n = len(row)
            for j, t in enumerate(row):
                if t == K + 1 or t == K + 2:
                    n = j + 1 if t == K + 1 else j
                    break
            out.append(n)
        return out

    def score_streams(self, phone, semantic, attention_mask=None, semantic_attention_mask=None, labels=None, append_eos=False):
        """The id arithmetic of `score` (no device work beyond the caller's tensors): -> (ids [B, S] the right-padded streams, their lengths as a
        list, labels [B, S] for lds_llama_score or None = ids, at [B, T (+ 1)] the stream position that predicts semantic token j, valid
        [B, T (+ 1)] whether row b has a token j)"""
        K, shift = self.cfg["semantic_kmeans_num"], self.semantic_token_shift
        if semantic.dim() != 2 or semantic.shape[0] != phone.shape[0] or semantic.shape[1] < 1:
            raise ValueError(f"semantic must be [B, T] with B = {phone.shape[0]} and T >= 1, got {tuple(semantic.shape)}")
        B, T = semantic.shape
        stream_labels = isinstance(labels, str)
        if stream_labels and labels != "stream":
            raise ValueError(f"labels must be None, 'stream' or a [B, T] tensor, got {labels!r}")
        if labels is not None and not stream_labels and tuple(labels.shape) != (B, T):
            raise ValueError(f"labels must have semantic's shape {(B, T)}, got {tuple(labels.shape)}")
        sl = self.semantic_lengths(semantic, semantic_attention_mask)
        sem = semantic.detach().to("cpu", torch.int64)
        tails, tl = [], []
        for b, n in enumerate(sl):
            body = sem[b, :n]
            if bool(((body < 0) | (body > K + 2)).any()):
                raise ValueError(f"row {b}: semantic ids inside the length must lie in 0 .. {K + 2}")
            tail = [torch.tensor([self.cfg["bos"]]), body + shift] + ([torch.tensor([self.cfg["eos"]])] if append_eos else [])
            tails.append(torch.cat(tail))
            tl.append(n + (1 if append_eos else 0))
            if tl[-1] < 1:
                raise ValueError(f"row {b}: no semantic token to score")
        ids, lens, nph = self._streams(phone, attention_mask, tails)
        S, Tout = ids.shape[1], T + (1 if append_eos else 0)
        if S > self.cfg["max_pos"]:
            raise ValueError(f"the longest stream has {S} ids, max_position_embeddings is {self.cfg['max_pos']}")
        dev = ids.device
        # token j of row b is id nph[b] + 3 + j of the stream, predicted at position nph[b] + 2 + j
        first = torch.tensor(nph, device=dev)[:, None] + 2
        j = torch.arange(Tout, device=dev)[None]
        valid = j < torch.tensor(tl, device=dev)[:, None]
        at = torch.where(valid, first + j, torch.zeros_like(j))      # [B, Tout] indices into [B, S - 1]
        if stream_labels:
            lab = None      # = input_ids
        else:
            lab = torch.full_like(ids, -100)
            tgt = ids.gather(1, at + 1)
            if labels is not None:
                given = labels.to(device=dev, dtype=torch.int64)
                if bool((valid[:, :T] & (given != -100) & ((given < 0) | (given > K + 2))).any()):
                    raise ValueError(f"labels inside the lengths must be -100 or lie in 0 .. {K + 2}")
                keep = torch.ones_like(valid)
                keep[:, :T] = given != -100
                tgt = tgt.clone()
                tgt[:, :T] = torch.where(given != -100, given + shift, tgt[:, :T])
                tgt = torch.where(keep, tgt, torch.full_like(tgt, -100))
            lab.scatter_(1, torch.where(valid, at + 1, torch.zeros_like(at)), torch.where(valid, tgt, lab[:, :1].expand_as(tgt)))
            lab[:, 0] = -100      # (the slot the rows behind their ends were pointed at; position 0 is never a target)
        return ids, lens, lab, at, valid

    @torch.no_grad()
    def score(self, phone, tone, semantic, attention_mask=None, semantic_attention_mask=None, labels=None, append_eos=False, return_logits=False):
        """Teacher-forced scoring of the semantic part of the stream.  semantic [B, T] is in the numbering `generate` returns (token t, EOS =
        K + 1, pad = K + 2; no BOS); row b's stream is [108, phones_b, 109, 108 + K, semantic_b + 108] with the semantic EOS appended when
        append_eos -- the reference `forward`'s stream (llama.py:98-101).  A row's tokens end as `semantic_lengths` says.  `tone` has no
        effect, as in `generate`.
        Returns an LMScore whose arrays run per semantic token, [B, T] ([B, T + 1] with append_eos): entry j is the log-probability and the
        rank, over the full vocabulary, of token j given everything before it (0 / -1 behind a row's end and where the label is -100);
        seq_logprob [B] their sums.  labels: None = the semantic targets only (loss = their mean negative log-probability: reranking);
        "stream" = every id of the stream, phones included (loss = the reference's training loss, labels = input_ids); a [B, T] tensor in
        semantic's numbering with -100 holes (an appended EOS stays a target).  With return_logits, logits [B, T (+ 1), K + 3] are the raw logits
        of the ids 108 .. vocab that predict token j: `generate(..., return_logits=True)`'s, bit for bit, for tokens that `generate` produced."""
        ids, lens, lab, at, valid = self.score_streams(phone, semantic, attention_mask, semantic_attention_mask, labels, append_eos)
        if not (phone.is_cuda and semantic.is_cuda):
            raise RuntimeError("Llama.score needs tensors on a HIP device (no CPU fallback)")
        B, dev, shift = ids.shape[0], ids.device, self.semantic_token_shift
        ids_len = torch.tensor(lens, dtype=torch.int32, device=dev)
        lp, ranks, loss, n, logits = self.native().score(ids, ids_len, lab, return_logits)
        tok_lp = torch.where(valid, lp.gather(1, at), torch.zeros_like(lp[:, :1]))
        tok_rk = torch.where(valid, ranks.gather(1, at), torch.full_like(ranks[:, :1], -1))
        out_logits = None
        if return_logits:
            picked = logits[torch.arange(B, device=dev)[:, None], at][:, :, shift:]
            out_logits = torch.where(valid[:, :, None], picked, torch.zeros_like(picked))
        return LMScore(loss, tok_lp, tok_rk, tok_lp.double().sum(-1).float(), n, out_logits)

    @torch.no_grad()
    def generate(self, phone, tone, attention_mask=None, use_cache=None, max_length=1024, do_sample=True, temperature=1.0, top_k=5, top_p=1.0,
                 repetition_penalty=1.0, num_beams=1, no_repeat_ngram_size=0, early_stopping=True, spk_id=None, end_gate_threshold=None,
                 return_logits=False, uniforms=None, semantic_prompt=None, prompt_attention_mask=None, **kwargs):
        """The reference's `generate` (llama.py:121-184): phone [1, L] -> the generated semantic ids [1, n] (shift subtracted, EOS = K + 1 kept);
        max_length is the total length, the L + 3 prompt ids included.  tone, spk_id and use_cache have no effect, as there; early_stopping is forced off with one
        beam (llama.py:154).
        num_beams 2 .. 8 with do_sample=False: HF's greedy beam search (length_penalty 1) with the caller's early_stopping (True, False or "never"):
        log_softmax over the whole vocabulary, then the repetition penalty, the n-gram ban and the ban of the ids below 108; a row's
        decoder_prompt_len is its own stream length, semantic prompt included.  Rows of a batch equal the rows alone.  Not built: beam sampling
        (do_sample=True, the default), return_logits with beams.
        Extensions: phone [B, L] with a right-padded attention_mask [B, L] (ones then zeros; the reference can only do B = 1 and hands its mask to
        nothing that reads it): row b is [108, phones_b, 109, 108 + K] with its own length and decodes exactly as it would alone; returned rows
        are cropped to the longest and padded with K + 2.  return_logits: also logits [steps, B, K + 3], logits[s][b] = HF's raw logits (before
        any processor) of the ids 108 .. vocab that chose row b's s-th generated token.  uniforms [max_length - 1, B] (sampling): row b's s-th
        generated token uses uniforms[s][b]; None draws them with torch.rand.
        semantic_prompt [B, P] int64 in the returned numbering, the semantic BOS (K) first like Roformer.generate's, right-padded with
        prompt_attention_mask [B, P] (ones then zeros) when the rows' prompts differ in length: row b's stream is [108, phones_b, 109,
        semantic_prompt_b + 108] and the decode continues it -- a voice or prosody prompt, or the previous sentence's tail.  The returned rows
        stay "the ids behind the semantic BOS, minus 108": they begin with the prompt's tokens.  max_length counts everything; the repetition
        penalty and the n-gram ban see the prompt, as HF would; logits[s][b] chose row b's s-th GENERATED token."""
        if end_gate_threshold is not None:
            # reference llama.py:11-20 sets the WHOLE score row to +inf once softmax(scores)[eos] passes the threshold: greedy then picks
            # id 0 and sampling makes torch.multinomial raise on NaN probabilities -- there is no coherent behaviour to restate
            raise NotImplementedError("the end gate is not built: the reference's EndGateLogitsProcessor sets the whole score row to +inf, "
                                      "after which greedy picks token 0 and sampling raises")
        if isinstance(num_beams, bool) or not isinstance(num_beams, (int, np.integer)) or not 1 <= num_beams <= 8:
            raise ValueError(f"num_beams must be an integer in 1 .. 8, got {num_beams!r}")
        if num_beams > 1:
            if do_sample:
                raise NotImplementedError("beam sampling (num_beams > 1 with do_sample=True, the default) is not built: greedy beam search takes do_sample=False")
            if return_logits:
                raise NotImplementedError("return_logits is not available with beam search (num_beams > 1)")
            if not (early_stopping is True or early_stopping is False or early_stopping == "never"):
                raise ValueError(f"early_stopping must be True, False or 'never', got {early_stopping!r}")
            if self.cfg["vocab"] > 4352:
                raise NotImplementedError(f"beam search is built for vocabularies of at most 4352 ids (K <= 4241), got {self.cfg['vocab']}")
        if isinstance(no_repeat_ngram_size, bool) or not isinstance(no_repeat_ngram_size, (int, np.integer)) or no_repeat_ngram_size < 0:
            raise ValueError(f"no_repeat_ngram_size must be an integer >= 0, got {no_repeat_ngram_size!r}")
        top_k = 0 if top_k is None else int(top_k)
        if do_sample and not (0 <= top_k <= 64):
            raise NotImplementedError("sampling is built for top_k = None / 0 (no filter) or 1 <= top_k <= 64")
        if semantic_prompt is None and prompt_attention_mask is not None:
            raise ValueError("prompt_attention_mask needs semantic_prompt")
        if semantic_prompt is None:
            ids, lens = self.input_ids(phone, attention_mask)
            first = lens      # where each row's returned ids begin: behind the semantic BOS
        else:      # everything about the prompt is checked before any device work
            tails = self._check_prompt(phone.shape[0], semantic_prompt, prompt_attention_mask)
            ids, lens, nph = self._streams(phone, attention_mask, tails)
            first = [n + 3 for n in nph]
        B = ids.shape[0]
        if B > 64:
            raise ValueError(f"a Llama decode takes at most 64 rows, got {B}")
        if num_beams > 1 and B * num_beams > 256:
            raise ValueError(f"a Llama beam decode takes at most 256 beam rows, got B * num_beams = {B * num_beams}")
        if num_beams > 1 and max_length > 7488:
            raise ValueError(f"a Llama beam decode takes max_length <= 7488, got {max_length}")
        for b, n in enumerate(lens):
            if n >= max_length:      # HF raises ValueError as well: max_length counts the prompt
                raise ValueError(f"row {b}: the prompt has {n} ids (phones + 3" + (f" + {n - first[b]} prompt tokens" if n > first[b] else "") +
                                 f"), which leaves no room below max_length = {max_length} (the total length)")
        if max_length > self.cfg["max_pos"]:
            raise ValueError(f"max_length = {max_length} exceeds max_position_embeddings = {self.cfg['max_pos']}")
        if not phone.is_cuda:
            raise RuntimeError("Llama.generate needs tensors on a HIP device (no CPU fallback)")
        if not do_sample:
            uniforms = None
        elif uniforms is None:
            uniforms = torch.rand(max_length - 1, B, device=ids.device)      # one draw per step and sequence
        else:
            uniforms = uniforms.to(device=ids.device, dtype=torch.float32)
            if uniforms.dim() != 2 or uniforms.shape[1] != B or uniforms.shape[0] < max_length - min(lens):
                raise ValueError(f"uniforms must be [steps, B = {B}] with one row per generated position, got {tuple(uniforms.shape)}")
            if uniforms.shape[0] < max_length - 1:      # the library's layout is [max_length - 1, B]; the rows past the last step are never read
                uniforms = torch.cat([uniforms, uniforms.new_zeros(max_length - 1 - uniforms.shape[0], B)])
        if num_beams > 1:      # every item's prompt and best finished hypothesis: EOS kept (a hypothesis without one ends at max_length), pad after it
            toks, logits = self.native().generate_beam(ids, lens, max_length, int(num_beams), repetition_penalty, int(no_repeat_ngram_size), early_stopping), None
        else:
            toks, logits = self.native().generate(ids, lens, max_length, do_sample, top_k, top_p, temperature, repetition_penalty, uniforms, return_logits,
                                                  no_repeat_ngram_size=int(no_repeat_ngram_size))
        # llama.py:182 for every row: the ids behind the row's own prompt, cropped to the longest row, padded with the pad id; then the shift
        host = toks.cpu()
        ends = []
        for b, n in enumerate(lens):      # a row ends with its first EOS behind the prompt, else with the returned rows
            hit = (host[b, n:] == self.cfg["eos"]).nonzero()
            ends.append(n + int(hit[0]) + 1 if hit.numel() else toks.shape[1])
        out = torch.full((B, max(e - n for e, n in zip(ends, first))), self.cfg["pad"], dtype=torch.int64, device=toks.device)
        for b, (e, n) in enumerate(zip(ends, first)):
            out[b, : e - n] = toks[b, n:e]
        out = out - self.semantic_token_shift
        return (out, logits) if return_logits else out
