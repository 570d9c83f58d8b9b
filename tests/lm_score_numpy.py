"""Teacher-forced LM scoring restated in numpy over oracle.roformer's functions: the decoder evaluated at ALL positions of a given token
sequence with a causal self-attention (query t sees keys 0 .. t) -- the prefix evaluation that tests/golden/make_lm_score_fixtures.py
records from the reference, and what oracle.roformer.decoder_step computes one token at a time.  Statistics in float64 as the recipe takes
them."""
import math

import numpy as np

from oracle import roformer as R

f32 = np.float32
IGNORE = -100


def causal_logits(w, cfg, enc, semantic, enc_len=None):
    """enc [B,L,hidden] (encoder states), semantic [B,T] int (ids already valid) -> logits [B,T,V] fp32"""
    p = "semantic_decoder.roformer."
    H = cfg["heads"]
    x = R.layer_norm(w[p + "embeddings.word_embeddings.weight"][semantic] + w[p + "embeddings.token_type_embeddings.weight"][0],
                     w[p + "embeddings.LayerNorm.weight"], w[p + "embeddings.LayerNorm.bias"], cfg["eps"])
    table = w[p + "encoder.embed_positions.weight"]
    kv = R.cross_kv(w, cfg, enc)
    T = semantic.shape[1]
    future = np.triu(np.ones((T, T), dtype=bool), 1)
    for i in range(cfg["dec_layers"]):
        q = p + f"encoder.layer.{i}."
        a = q + "attention."
        qh = R.rotary(R.heads(R.linear(x, w[a + "self.query.weight"], w[a + "self.query.bias"]), H), table, 0)
        kh = R.rotary(R.heads(R.linear(x, w[a + "self.key.weight"], w[a + "self.key.bias"]), H), table, 0)
        vh = R.heads(R.linear(x, w[a + "self.value.weight"], w[a + "self.value.bias"]), H)
        s = np.matmul(qh, kh.transpose(0, 1, 3, 2)).astype(f32) / f32(math.sqrt(qh.shape[-1]))
        s = np.where(future[None, None], f32(-np.inf), s).astype(f32)
        s = s - s.max(-1, keepdims=True)
        pr = np.exp(s).astype(f32)
        pr = (pr / pr.sum(-1, keepdims=True)).astype(f32)
        o = np.matmul(pr, vh).astype(f32)
        B, _, _, d = o.shape
        ctx = o.transpose(0, 2, 1, 3).reshape(B, T, H * d)
        x = R.layer_norm(R.linear(ctx, w[a + "output.dense.weight"], w[a + "output.dense.bias"]) + x, w[a + "output.LayerNorm.weight"],
                         w[a + "output.LayerNorm.bias"], cfg["eps"])
        x = R._cross_attention(w, q + "crossattention.", cfg, x, kv[i], enc_len)
        x = R._ffn(w, q, cfg, x)
    c = "semantic_decoder.cls.predictions."
    t = R.layer_norm(R.gelu(R.linear(x, w[c + "transform.dense.weight"], w[c + "transform.dense.bias"])), w[c + "transform.LayerNorm.weight"],
                     w[c + "transform.LayerNorm.bias"], cfg["eps"])
    return R.linear(t, w[c + "decoder.weight"], w[c + "decoder.bias"])


def statistics(logits, labels, sem_len=None):
    """lp [B,T-1] float64 (0 where not counted), rank [B,T-1] int32 (-1 where not counted), loss, n_counted"""
    B, T, _ = logits.shape
    sem_len = np.full(B, T) if sem_len is None else np.asarray(sem_len)
    lp = np.zeros((B, T - 1))
    rank = np.full((B, T - 1), -1, dtype=np.int32)
    for b in range(B):
        for t in range(T - 1):
            y = int(labels[b, t + 1])
            if t + 1 >= sem_len[b] or y == IGNORE:
                continue
            row = logits[b, t].astype(np.float64)
            mx = row.max()
            lp[b, t] = row[y] - (mx + np.log(np.exp(row - mx).sum()))
            rank[b, t] = int((row > row[y]).sum() + (row[:y] == row[y]).sum())
    n = int((rank >= 0).sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        loss = np.float64(-lp.sum()) / np.float64(n)
    return lp, rank, loss, n


def score(w, cfg, phone, tone, spk_id, semantic, labels=None, sem_len=None, enc_len=None):
    """the whole entry: encoder, causal decoder, statistics.  Ids at and beyond a row's length are replaced by 0 (never counted)."""
    B, T = semantic.shape
    sl = np.full(B, T) if sem_len is None else np.asarray(sem_len)
    sem = np.where(np.arange(T)[None, :] < sl[:, None], semantic, 0)
    enc = R.encoder_forward(w, cfg, phone, tone, spk_id, enc_len)
    logits = causal_logits(w, cfg, enc, sem, enc_len)
    return (logits,) + statistics(logits, semantic if labels is None else labels, sl)
