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

Scope: phone mode, inference, num_beams 1 (greedy and sampling, each with the repetition penalty and n-gram blocking).
Not built (each raises): mode 'text', the end gate, beam search, `forward` (training), attention_bias / mlp_bias, a rope type other than
default, hidden_act other than silu."""
import numpy as np
import torch

from lds import arch, native
from lds.paramtree import ParamTree
from text2semantic.roformer.roformer import _get


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

    @torch.no_grad()
    def generate(self, phone, tone, attention_mask=None, use_cache=None, max_length=1024, do_sample=True, temperature=1.0, top_k=5, top_p=1.0,
                 repetition_penalty=1.0, num_beams=1, no_repeat_ngram_size=0, early_stopping=True, spk_id=None, end_gate_threshold=None,
                 return_logits=False, uniforms=None, **kwargs):
        """The reference's `generate` (llama.py:121-184): phone [1, L] -> the generated semantic ids [1, n] (shift subtracted, EOS = K + 1 kept);
        max_length is the total length, the L + 3 prompt ids included.  tone, spk_id, use_cache and early_stopping (forced off with one beam,
        llama.py:154) have no effect, as there.
        Extensions: phone [B, L] with a right-padded attention_mask [B, L] (ones then zeros; the reference can only do B = 1 and hands its mask to
        nothing that reads it): row b is [108, phones_b, 109, 108 + K] with its own length and decodes exactly as it would alone; returned rows
        are cropped to the longest and padded with K + 2.  return_logits: also logits [steps, B, K + 3], logits[s][b] = HF's raw logits (before
        any processor) of the ids 108 .. vocab that chose row b's s-th generated token.  uniforms [max_length - 1, B] (sampling): row b's s-th
        generated token uses uniforms[s][b]; None draws them with torch.rand."""
        if end_gate_threshold is not None:
            # reference llama.py:11-20 sets the WHOLE score row to +inf once softmax(scores)[eos] passes the threshold: greedy then picks
            # id 0 and sampling makes torch.multinomial raise on NaN probabilities -- there is no coherent behaviour to restate
            raise NotImplementedError("the end gate is not built: the reference's EndGateLogitsProcessor sets the whole score row to +inf, "
                                      "after which greedy picks token 0 and sampling raises")
        if isinstance(num_beams, bool) or not isinstance(num_beams, (int, np.integer)) or num_beams < 1:
            raise ValueError(f"num_beams must be an integer >= 1, got {num_beams!r}")
        if num_beams > 1:
            # HF normalises with log_softmax over the whole vocabulary before the processors: the head would have to give the banned columns' share
            raise NotImplementedError("beam search (num_beams > 1) is not built for Llama; Roformer.generate has greedy beam search")
        if isinstance(no_repeat_ngram_size, bool) or not isinstance(no_repeat_ngram_size, (int, np.integer)) or no_repeat_ngram_size < 0:
            raise ValueError(f"no_repeat_ngram_size must be an integer >= 0, got {no_repeat_ngram_size!r}")
        top_k = 0 if top_k is None else int(top_k)
        if do_sample and not (0 <= top_k <= 64):
            raise NotImplementedError("sampling is built for top_k = None / 0 (no filter) or 1 <= top_k <= 64")
        ids, lens = self.input_ids(phone, attention_mask)
        B = ids.shape[0]
        if B > 64:
            raise ValueError(f"a Llama decode takes at most 64 rows, got {B}")
        for b, n in enumerate(lens):
            if n >= max_length:      # HF raises ValueError as well: max_length counts the prompt
                raise ValueError(f"row {b}: the prompt has {n} ids (phones + 3), which leaves no room below max_length = {max_length} (the total length)")
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
        toks, logits = self.native().generate(ids, lens, max_length, do_sample, top_k, top_p, temperature, repetition_penalty, uniforms, return_logits,
                                              no_repeat_ngram_size=int(no_repeat_ngram_size))
        # llama.py:182 for every row: the ids behind the row's own prompt, cropped to the longest row, padded with the pad id; then the shift
        host = toks.cpu()
        ends = []
        for b, n in enumerate(lens):      # a row ends with its first EOS behind the prompt, else with the returned rows
            hit = (host[b, n:] == self.cfg["eos"]).nonzero()
            ends.append(n + int(hit[0]) + 1 if hit.numel() else toks.shape[1])
        out = torch.full((B, max(e - n for e, n in zip(ends, lens))), self.cfg["pad"], dtype=torch.int64, device=toks.device)
        for b, (e, n) in enumerate(zip(ends, lens)):
            out[b, : e - n] = toks[b, n:e]
        out = out - self.semantic_token_shift
        return (out, logits) if return_logits else out
