"""The text2semantic Llama (reference text2semantic/llama/llama.py over HF LlamaForCausalLM + GenerationMixin) restated in numpy: fp32 storage
(weights, and every activation a kernel would store), float64 accumulation inside each operation.

  RMSNorm          (x * rsqrt(mean(x^2) + eps)) * w
  attention        bias-free q / k / v / o, query head h reads kv head h // (heads // kv_heads), scale head_dim^-0.5, causal through the cache
  rotary           half-split (element i pairs with i + d/2); the angle is the FP32 product of position and inv_freq, as HF forms it -- an angle
                   formed in double is about 6e-5 rad away at position 1000.  inv_freq is an argument: HF's own numbers (torch's fp32 pow)
  MLP              down(silu(gate x) * up x)
  generate         llama.py:121-184 for one row: ids = [108, phones, 109, 108 + K]; per step, on the raw logits of the last position, HF's order:
                   repetition penalty -> n-gram ban (both over the WHOLE ids, phones included) -> the ban of the ids below 108 -> temperature ->
                   top-k -> top-p -> the inverse-CDF draw.  The banned columns are simply left out: only the K + 3 columns from 108 on are formed,
                   the history is looked at in shifted ids (phone ids are negative there: never a candidate, but part of the n-gram contexts)."""
import numpy as np

from oracle import roformer as R

from lm_beam_numpy import ngram_banned

f32, f64 = np.float32, np.float64


def rope_tables(inv_freq, n_pos):
    ang = (np.arange(n_pos, dtype=f32)[:, None] * np.asarray(inv_freq, dtype=f32)[None, :]).astype(f32)      # the fp32 product
    return np.cos(ang.astype(f64)).astype(f32), np.sin(ang.astype(f64)).astype(f32)


def _rms(x, w, eps):
    x = x.astype(f64)
    return ((x / np.sqrt((x * x).mean() + eps)) * w.astype(f64)).astype(f32)


def _lin(w, x):
    return (w.astype(f64) @ x.astype(f64)).astype(f32)


def _rot(x, cos, sin):      # x [heads, d]; cos, sin [d/2]
    x = x.astype(f64)
    h = x.shape[-1] // 2
    x1, x2 = x[:, :h], x[:, h:]
    return np.concatenate([x1 * cos - x2 * sin, x2 * cos + x1 * sin], axis=-1).astype(f32)


class Decoder:
    """the cached decoder: step(id) appends one position and returns the raw logits of the columns cfg['shift'] .. vocab (fp32)"""

    def __init__(self, w, cfg, inv_freq):
        self.w, self.cfg = w, cfg
        self.cos, self.sin = rope_tables(inv_freq, cfg["max_pos"])
        self.k = [[] for _ in range(cfg["layers"])]
        self.v = [[] for _ in range(cfg["layers"])]
        self.pos = 0
        self.head = np.ascontiguousarray(w["llama.lm_head.weight"][cfg["shift"]:])

    def step(self, tok, want_logits=True):
        w, c = self.w, self.cfg
        H, nh, nkv, d = c["hidden"], c["heads"], c["kv_heads"], c["head_dim"]
        tok = min(max(int(tok), 0), c["vocab"] - 1)
        x = w["llama.model.embed_tokens.weight"][tok].astype(f32)
        cos, sin = self.cos[self.pos].astype(f64), self.sin[self.pos].astype(f64)
        for i in range(c["layers"]):
            p = f"llama.model.layers.{i}."
            h = _rms(x, w[p + "input_layernorm.weight"], c["eps"])
            q = _rot(_lin(w[p + "self_attn.q_proj.weight"], h).reshape(nh, d), cos, sin)
            k = _rot(_lin(w[p + "self_attn.k_proj.weight"], h).reshape(nkv, d), cos, sin)
            v = _lin(w[p + "self_attn.v_proj.weight"], h).reshape(nkv, d)
            self.k[i].append(k)
            self.v[i].append(v)
            K, V = np.stack(self.k[i]).astype(f64), np.stack(self.v[i]).astype(f64)      # [T, nkv, d]
            ctx = np.empty((nh, d), dtype=f32)
            for hh in range(nh):
                g = hh // (nh // nkv)
                s = (K[:, g] @ q[hh].astype(f64)) * (d ** -0.5)
                e = np.exp(s - s.max())
                ctx[hh] = ((e / e.sum()) @ V[:, g]).astype(f32)
            x = (x.astype(f64) + _lin(w[p + "self_attn.o_proj.weight"], ctx.reshape(-1)).astype(f64)).astype(f32)
            h = _rms(x, w[p + "post_attention_layernorm.weight"], c["eps"])
            gte, up = _lin(w[p + "mlp.gate_proj.weight"], h).astype(f64), _lin(w[p + "mlp.up_proj.weight"], h).astype(f64)
            ff = ((gte / (1.0 + np.exp(-gte))) * up).astype(f32)
            x = (x.astype(f64) + _lin(w[p + "mlp.down_proj.weight"], ff).astype(f64)).astype(f32)
        self.pos += 1
        if not want_logits:
            return None
        return _lin(self.head, _rms(x, w["llama.model.norm.weight"], c["eps"]))


def prompt_ids(cfg, phones):
    return [cfg["text_bos"]] + [int(t) for t in phones] + [cfg["text_eos"], cfg["bos"]]


def choose(lg, hist, do_sample=False, top_k=5, top_p=1.0, temperature=1.0, repetition_penalty=1.0, no_repeat_ngram_size=0, u=None):
    """one token choice on the raw logits `lg` of the K + 3 columns; hist = the whole ids so far, SHIFTED.  Returns (shifted token, margin): the
    top-1 / top-2 gap of the processed scores (greedy) or the distance of u from the nearest CDF step and the k | k + 1 score gap (sampling)."""
    V = lg.shape[0]
    s = np.asarray(lg, dtype=f32).copy()
    if repetition_penalty != 1.0:
        for t in sorted(set(int(t) for t in hist)):
            if 0 <= t < V:
                s[t] = s[t] * f32(repetition_penalty) if s[t] < 0 else s[t] / f32(repetition_penalty)
    for t in ngram_banned(hist, no_repeat_ngram_size):
        if 0 <= t < V:
            s[t] = -np.inf
    if not do_sample:
        o = np.sort(s)[::-1]
        return int(np.argmax(s)), float(o[0] - o[1])
    tok, cdf = R.pick_token_hf(s, [], top_k, top_p, temperature, 1.0, u, with_cdf=True)
    margin = float(np.abs(cdf.astype(f64) - f64(f32(u))).min())
    if top_k:
        o = np.sort(s)[::-1]
        if np.isfinite(o[top_k]):
            margin = min(margin, float(o[top_k - 1] - o[top_k]))
    return tok, margin


def generate_row(w, cfg, inv_freq, ids, max_length, uniforms=None, **kw):
    """ids: the row's prompt (model ids; prompt_ids(cfg, phones), possibly followed by generated ids).  Returns (ids [n] with the prompt in
    front, EOS kept; logits [n - P, K + 3]; margins [n - P])."""
    ids = [int(t) for t in ids]
    if len(ids) >= max_length:
        raise ValueError(f"the prompt has {len(ids)} ids, max_length is {max_length}")
    dec = Decoder(w, cfg, inv_freq)
    for t in ids[:-1]:
        dec.step(t, want_logits=False)
    seq, out, margins = list(ids), [], []
    while len(seq) < max_length:
        lg = dec.step(seq[-1])
        tok, m = choose(lg, [t - cfg["shift"] for t in seq], u=None if uniforms is None else uniforms[len(out)], **kw)
        out.append(lg)
        margins.append(m)
        seq.append(tok + cfg["shift"])
        if seq[-1] == cfg["eos"]:
            break
    return np.array(seq, dtype=np.int64), np.stack(out), np.array(margins)
