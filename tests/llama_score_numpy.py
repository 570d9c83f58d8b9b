"""Teacher-forced scoring under the text2semantic Llama restated in numpy, on top of tests/llama_numpy.py's cached decoder: the logits of
every position of a stream over the WHOLE vocabulary (the decoder stepped through the stream's ids, the head un-sliced), and HF's shifted
cross entropy with lds_llama_score's definitions (include/lds.h): position t is counted when t + 1 lies inside the row and labels[t + 1] is a
vocabulary id; lp = logit_y - logsumexp, rank = the columns above the label's logit with ties to the lowest index; loss = the mean of -lp
over the counted positions of the whole batch."""
import numpy as np

import llama_numpy as LN

f32, f64 = np.float32, np.float64


def stream_logits(w, cfg, inv_freq, ids):
    """ids [S] (model ids) -> logits [S, vocab] fp32: row t from the prefix ids[:t + 1]"""
    dec = LN.Decoder(w, cfg, inv_freq)
    dec.head = np.ascontiguousarray(w["llama.lm_head.weight"])      # every column, the ids below the shift included
    return np.stack([dec.step(t) for t in ids])


def stream(cfg, phones, semantic, append_eos=False):
    """[108, phones, 109, 108 + K, semantic + 108, (EOS)] (reference llama.py:94-101)"""
    tail = [cfg["eos"]] if append_eos else []
    return np.array(LN.prompt_ids(cfg, phones) + [int(t) + cfg["shift"] for t in semantic] + tail, dtype=np.int64)


def semantic_length(cfg, row):
    """a row of `generate`'s output ends behind its first EOS (K + 1, kept) or before its first pad (K + 2)"""
    K = cfg["semantic_kmeans_num"]
    for j, t in enumerate(row):
        if t == K + 1:
            return j + 1
        if t == K + 2:
            return j
    return len(row)


def row_stats(logits, labels, length=None):
    """logits [S, V], labels [S] -> (lp [S - 1] fp32, rank [S - 1] int32): 0 / -1 where position t is not counted"""
    S, V = logits.shape
    length = S if length is None else min(int(length), S)
    lp, rank = np.zeros(S - 1, f32), np.full(S - 1, -1, np.int32)
    for t in range(S - 1):
        y = int(labels[t + 1]) if t + 1 < length else -100
        if not 0 <= y < V:
            continue
        row = logits[t].astype(f64)
        m = row.max()
        lp[t] = f32(row[y] - (m + np.log(np.exp(row - m).sum())))
        rank[t] = int((row > row[y]).sum() + (row[:y] == row[y]).sum())
    return lp, rank


def score_ids(w, cfg, inv_freq, ids, lens=None, labels=None):
    """ids [B, S] right-padded, lens [B] or None, labels [B, S] or None (= ids) -> (lp [B, S - 1], rank [B, S - 1], loss, n_counted,
    logits [B, S, vocab] with the rows behind a length left at zero)"""
    ids = np.asarray(ids)
    B, S = ids.shape
    lens = [S] * B if lens is None else [int(v) for v in lens]
    labels = ids if labels is None else np.asarray(labels)
    lp, rank = np.zeros((B, S - 1), f32), np.full((B, S - 1), -1, np.int32)
    logits = np.zeros((B, S, cfg["vocab"]), f32)
    for b in range(B):
        logits[b, :lens[b]] = stream_logits(w, cfg, inv_freq, ids[b, :lens[b]])
        lp[b], rank[b] = row_stats(logits[b], labels[b], lens[b])
    n = int((rank >= 0).sum())
    loss = float(-lp[rank >= 0].astype(f64).sum() / n) if n else float("nan")
    return lp, rank, loss, n, logits
