"""Whisper's text decoder restated in numpy (OpenAI whisper/model.py TextDecoder over the reference's ResidualAttentionBlock(cross_attention=
True), encoder/whisper/model.py:42-110): float64 by default, float32 on request.  No caches: a greedy decode evaluates the whole sequence
again at every step.  Also the head's token choice with suppress lists and log-probs (csrc/whisper_dec.hip's definitions), and the
seeded inputs that the fixtures, the CPU tests and the GPU tests share (the fixtures store results, not inputs)."""
import math

import numpy as np

try:
    from scipy.special import erf as _erf
except Exception:      # pragma: no cover
    _erf = np.frompyfunc(math.erf, 1, 1)

# n_state / heads / layers, n_vocab, n_text_ctx (tests/golden/make_whisper_decoder_fixtures.py holds the same table)
CONFIGS = {
    "A": dict(n_state=128, n_head=2, n_layer=2, n_vocab=1031, n_text_ctx=32, max_new=40),
    "B": dict(n_state=192, n_head=3, n_layer=1, n_vocab=320, n_text_ctx=448, max_new=10),
    "C": dict(n_state=1280, n_head=20, n_layer=1, n_vocab=2053, n_text_ctx=448, max_new=8),
}
N_FRAMES = (1, 37, 100)
PROMPT_LEN = (1, 2, 4)
TF_S = 9
TF_LEN = (9, 5, 2)
T_PAD = 100            # frames of the batch's units buffer
T_LONG = 1500          # A's extra single-row case


def inputs(name, uniform, seed):
    """The seeded inputs of configuration `name`: units [3][T_PAD][C] (rows beyond N_FRAMES are part of the buffer and must not matter),
    units_long [1][T_LONG][C] (A only), teacher-forced tokens [3][TF_S], prompts (3 id lists), eos, suppress, begin_suppress.
    `uniform` is lds.init_weights.uniform."""
    c = CONFIGS[name]
    C, V = c["n_state"], c["n_vocab"]
    ids = lambda tag, shape: np.minimum((uniform(f"wdec.{name}.{tag}", shape, seed, 0.0, 1.0).astype(np.float64) * V).astype(np.int64), V - 1)
    d = dict(units=uniform(f"wdec.{name}.units", (3, T_PAD, C), seed, -1.7, 1.7), tf_tokens=ids("tf", (3, TF_S)))
    pr = ids("prompt", (3, max(PROMPT_LEN)))
    d["prompts"] = [pr[b, :PROMPT_LEN[b]].tolist() for b in range(3)]
    d["eos"] = V - 2
    d["suppress"] = sorted(set(ids("suppress", (7,)).tolist()) - {V - 2})
    d["begin_suppress"] = sorted({V - 2} | set(ids("begin", (3,)).tolist()))
    if name == "A":
        d["units_long"] = uniform(f"wdec.{name}.units_long", (1, T_LONG, C), seed, -1.7, 1.7)
    return d


def layer_norm(x, g, b, eps=1e-5):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + x.dtype.type(eps)) * g + b


def gelu(x):
    return (0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)).astype(np.float64))).astype(x.dtype)


def _attn(w, p, x, src, n_head, causal):
    q = x @ w[p + "query.weight"].T + w[p + "query.bias"]
    k = src @ w[p + "key.weight"].T
    v = src @ w[p + "value.weight"].T + w[p + "value.bias"]
    S, C = q.shape
    d = C // n_head
    scale = x.dtype.type(d ** -0.25)
    out = np.empty_like(q)
    for h in range(n_head):
        sl = slice(h * d, (h + 1) * d)
        qk = (q[:, sl] * scale) @ (k[:, sl] * scale).T
        if causal:
            qk = qk + np.triu(np.full((S, S), -np.inf, dtype=x.dtype), 1)
        qk = qk - qk.max(-1, keepdims=True)
        e = np.exp(qk)
        out[:, sl] = (e / e.sum(-1, keepdims=True)) @ v[:, sl]
    return out @ w[p + "out.weight"].T + w[p + "out.bias"]


def decoder_row(w, cfg, tokens, xa, dtype=np.float64):
    """tokens [S] ints, xa [T_b][C] (the row's own frames only) -> logits [S][V]"""
    w = {k: np.asarray(v, dtype=dtype) for k, v in w.items()} if next(iter(w.values())).dtype != dtype else w
    xa = np.asarray(xa, dtype=dtype)
    tokens = np.asarray(tokens, dtype=np.int64)
    x = w["decoder.token_embedding.weight"][tokens] + w["decoder.positional_embedding"][: len(tokens)]
    for i in range(cfg["n_layer"]):
        p = f"decoder.blocks.{i}."
        xn = layer_norm(x, w[p + "attn_ln.weight"], w[p + "attn_ln.bias"])
        x = x + _attn(w, p + "attn.", xn, xn, cfg["n_head"], True)
        x = x + _attn(w, p + "cross_attn.", layer_norm(x, w[p + "cross_attn_ln.weight"], w[p + "cross_attn_ln.bias"]), xa, cfg["n_head"], False)
        hdn = gelu(layer_norm(x, w[p + "mlp_ln.weight"], w[p + "mlp_ln.bias"]) @ w[p + "mlp.0.weight"].T + w[p + "mlp.0.bias"])
        x = x + hdn @ w[p + "mlp.2.weight"].T + w[p + "mlp.2.bias"]
    x = layer_norm(x, w["decoder.ln.weight"], w["decoder.ln.bias"])
    return x @ w["decoder.token_embedding.weight"].T


def cast(w, dtype):
    return {k: np.asarray(v, dtype=dtype) for k, v in w.items()}


def logits_batch(w, cfg, tokens, units, n_frames, tok_len=None, dtype=np.float64):
    """Whisper.logits on a ragged batch, every row as if alone; ids at and beyond tok_len[b] count as 0 (lds_whisper_decoder_logits)"""
    w = cast(w, dtype)
    tokens = np.array(tokens, dtype=np.int64)
    out = []
    for b in range(tokens.shape[0]):
        t = tokens[b].copy()
        if tok_len is not None:
            t[tok_len[b]:] = 0
        out.append(decoder_row(w, cfg, t, units[b, : n_frames[b]], dtype))
    return np.stack(out)


def choose(logits, suppress=()):
    """one row: (token = arg-max over the unsuppressed columns, ties to the lowest id; its log-softmax over them; their log-sum-exp)"""
    lg = np.array(logits, dtype=np.float64)
    if len(suppress):
        lg[np.asarray(list(suppress), dtype=np.int64)] = -np.inf
    tok = int(np.argmax(lg))      # (numpy's argmax returns the first maximum)
    m = lg[tok]
    lse = m + math.log(np.exp(lg - m).sum())
    return tok, float(m - lse), float(lse)


def top2_gap(logits, suppress=()):
    lg = np.array(logits, dtype=np.float64)
    if len(suppress):
        lg[np.asarray(list(suppress), dtype=np.int64)] = -np.inf
    a = np.partition(lg, -2)[-2:]
    return float(a[1] - a[0])


def greedy_row(w, cfg, units_row, prompt, max_new, eos, suppress=(), begin_suppress=(), cap=None, dtype=np.float64, forward=None):
    """Greedy decode of one row without caches.  Returns (tokens: the prompt + generated ids, EOS kept; the chosen ids' log-probs; every
    step's logits row [steps][V]; the smallest top-2 gap over |logits|max along the path).  A row stops at EOS, after max_new ids or when
    the sequence holds cap (default n_text_ctx) ids.  forward(tokens) -> logits [S][V] replaces the numpy pass (the torch oracle)."""
    cap = cfg["n_text_ctx"] if cap is None else cap
    if forward is None:
        w = cast(w, dtype)
        forward = lambda t: decoder_row(w, cfg, t, units_row, dtype)
    toks, lps, rows, margin = list(prompt), [], [], math.inf
    for step in range(max_new):
        if len(toks) >= cap:
            break
        lg = np.asarray(forward(toks), dtype=np.float64)[-1]
        ban = list(suppress) + (list(begin_suppress) if step == 0 else [])
        tok, lp, _ = choose(lg, ban)
        margin = min(margin, top2_gap(lg, ban) / float(np.abs(lg).max()))
        rows.append(lg)
        toks.append(tok)
        lps.append(lp)
        if tok == eos:
            break
    return toks, lps, np.stack(rows), margin


def pad_rows(rows, width, fill):
    out = np.full((len(rows), width), fill, dtype=np.int64 if isinstance(fill, int) else np.float64)
    for b, r in enumerate(rows):
        out[b, : len(r)] = r
    return out
