"""numpy restatement of the LM decode's n-gram ban and of one step of HF's greedy beam search (transformers generation/utils.py
_beam_search, length_penalty 1), in the state layout of lds_test_lm_beam_step (include/lds_test.h), and a whole beam-search decode
driven by it over oracle.roformer's cached decoder step.  fp32 throughout; top-k ties go to the lower (flat) index, as in csrc/lm.hip.
Shared by tests/test_cpu_lm_beam.py (checked against transformers' own helpers and the reference's tokens), tests/test_gpu_lm_beam.py
and tests/test_gpu_lm_long.py (the kernels against it)."""
import numpy as np

MASK = np.float32(-1.0e9)
ZERO = np.float32(-0.0)
MASKED = -5e8      # scores carrying one of the -1e9 masks: their order among themselves never reaches the output


def ngram_banned(hist, n):
    """NoRepeatNGramLogitsProcessor on one history (BOS included): the last token of every n-window whose first n - 1 tokens equal
    the history's last n - 1 tokens"""
    hist = [int(t) for t in hist]
    L = len(hist)
    if n <= 0 or L < n:
        return set()
    prefix = hist[L - n + 1:]
    return {hist[i + n - 1] for i in range(L - n + 1) if hist[i:i + n - 1] == prefix}


def log_softmax(x):
    x = x.astype(np.float32)
    m = x.max(-1, keepdims=True)
    return (x - m) - np.log(np.exp(x - m).sum(-1, keepdims=True, dtype=np.float32)).astype(np.float32)


def _top(x, k):
    """indices of the k largest, ties to the lower index"""
    return np.argsort(-x, kind="stable")[:k]


def _gap(x, ranks):
    """the smallest score gap between the (r)-th and (r + 1)-th largest of x over `ranks` (1-based r), leaving out masked scores
    (make_lm_beam_fixtures.Margins.note)"""
    m = min(len(x), max(ranks) + 1)
    s = np.sort(np.partition(x, len(x) - m)[len(x) - m:])[::-1]
    g = np.inf
    for r in ranks:
        if r < len(s) and s[r] > MASKED and np.isfinite(s[r - 1]):
            g = min(g, float(s[r - 1]) - float(s[r]))
    return g


def running(bits, early_stopping):
    """_beam_search_has_unfinished_sequences from a step's flag bits"""
    return bool(bits & 1) and (early_stopping != 1 or bool(bits & 2)) and bool(bits & 4)


def beam_step(logits, K, cur_len, max_length, eos, rep_pen, ngram, early_stopping, run_seq, run_score, fin_seq, fin_score, fin_flag, fin_len,
              unsat):
    """one step; early_stopping 1 = True, 0 = False, 2 = "never".  Arrays: logits [B*K, V]; run_seq, fin_seq [B*K, max_length] int64;
    run_score, fin_score [B*K] fp32; fin_flag, fin_len [B*K] int; unsat [B] int.  Returns the new state, parent [B*K], the step's
    flag bits (1: some item may improve, 2: some item has an unfinished slot, 4: some candidate did not hit the stopping criteria) and
    "gap", the smallest score gap at a selection of the step (top 2K of K * V: ranks 2K | 2K + 1 and K | K + 1; running beams: K | K + 1;
    finished merge: K | K + 1 and 1 | 2)."""
    R, V = logits.shape
    B = R // K
    lp = log_softmax(logits)
    for r in range(R):
        hist = run_seq[r, :cur_len]
        if rep_pen != 1.0:
            for t in set(int(t) for t in hist):
                lp[r, t] = lp[r, t] * np.float32(rep_pen) if lp[r, t] < 0 else lp[r, t] / np.float32(rep_pen)
        for t in ngram_banned(hist, ngram):
            lp[r, t] = -np.inf
    acc = (lp + run_score.astype(np.float32)[:, None]).astype(np.float32)
    out = dict(run_seq=run_seq.copy(), run_score=run_score.astype(np.float32).copy(), fin_seq=fin_seq.copy(), fin_score=fin_score.astype(np.float32).copy(),
               fin_flag=fin_flag.copy(), fin_len=fin_len.copy(), unsat=unsat.copy(), parent=np.zeros(R, np.int32))
    bits, gap = 0, np.inf
    for b in range(B):
        rows = slice(b * K, (b + 1) * K)
        flat = acc[rows].reshape(-1)
        sel = _top(flat, 2 * K)
        gap = min(gap, _gap(flat, [2 * K, K]))
        topv, topb, topt = flat[sel], sel // V, sel % V
        hit = (topt == eos) | (cur_len + 1 >= max_length)
        trl = np.array([topv[j] + (MASK if hit[j] else ZERO) for j in range(2 * K)], np.float32)
        run_j = _top(trl, K)
        all_fin = bool(fin_flag[rows].all())
        f = np.zeros(2 * K, np.float32)
        for j in range(2 * K):
            did = bool(hit[j]) and j < K
            v = np.float32(topv[j] / np.float32(cur_len))
            v = np.float32(v + (MASK if (all_fin and early_stopping == 1) else ZERO))
            v = np.float32(v + (ZERO if unsat[b] else MASK))
            v = np.float32(v + (ZERO if did else MASK))
            f[j] = v
        ms = np.concatenate([fin_score[rows].astype(np.float32), f])
        fin_j = _top(ms, K)
        gap = min(gap, _gap(trl, [K]), _gap(ms, [K, 1]))
        for k in range(K):
            r = b * K + k
            j = run_j[k]
            par = b * K + topb[j]
            out["run_seq"][r, :cur_len] = run_seq[par, :cur_len]
            out["run_seq"][r, cur_len] = topt[j]
            out["run_score"][r] = trl[j]
            out["parent"][r] = topb[j]
            m = fin_j[k]
            if m < K:
                src = b * K + m
                out["fin_seq"][r] = fin_seq[src]
                out["fin_score"][r], out["fin_flag"][r], out["fin_len"][r] = fin_score[src], fin_flag[src], fin_len[src]
            else:
                jj = m - K
                out["fin_seq"][r] = run_seq[b * K + topb[jj]]
                out["fin_seq"][r, cur_len] = topt[jj]
                out["fin_score"][r], out["fin_flag"][r], out["fin_len"][r] = ms[m], int(hit[jj] and jj < K), cur_len
        hyp = max_length - 1 if early_stopping == 2 else cur_len
        best = np.float32(out["run_score"][b * K] / np.float32(hyp))
        worst = out["fin_score"][rows].min()
        improve = any(best > (worst if out["fin_flag"][b * K + k] else MASK) for k in range(K))
        out["unsat"][b] = int(bool(unsat[b]) and improve)
        bits |= (1 if out["unsat"][b] else 0) | (0 if out["fin_flag"][rows].all() else 2) | (0 if hit.all() else 4)
    out["flags"] = bits
    out["gap"] = gap
    return out


def generate_beam(w, cfg, enc, K, max_length, rep_pen=1.0, ngram=0, early_stopping=1, enc_len=None):
    """greedy beam search over oracle.roformer.decoder_step the way HF's _beam_search drives it: beam_step on every step's logits, then
    the key/value caches reordered by parent (HF's _reorder_cache), until the step's flag bits say HF's loop ends.  enc [B, L, hidden]
    encoder states, enc_len [B] or None.  Returns (tokens [B, n]: slot 0 of every item's finished hypotheses, BOS first, cropped to the
    longest generated length, PAD after each one's end; the smallest decision margin of the run, as make_lm_beam_fixtures.Margins)."""
    from oracle import roformer as R
    B = enc.shape[0]
    N = B * K
    eos, bos, pad = cfg["sem_eos"], cfg["sem_bos"], cfg["sem_pad"]
    kv = [(np.repeat(k, K, axis=0), np.repeat(v, K, axis=0)) for k, v in R.cross_kv(w, cfg, enc)]
    el = None if enc_len is None else np.repeat(np.asarray(enc_len), K)
    caches = [dict() for _ in range(cfg["dec_layers"])]
    run_seq = np.full((N, max_length), pad, np.int64)
    run_seq[:, 0] = bos
    st = dict(run_seq=run_seq, run_score=np.tile(np.array([0.0] + [-1e9] * (K - 1), np.float32), B), fin_seq=run_seq.copy(),
              fin_score=np.full(N, -1e9, np.float32), fin_flag=np.zeros(N, np.int32), fin_len=np.zeros(N, np.int32), unsat=np.ones(B, np.int32))
    gap = np.inf
    for step in range(max_length - 1):
        lg = R.decoder_step(w, cfg, st["run_seq"][:, step], step, caches, kv, el)
        out = beam_step(lg, K, step + 1, max_length, eos, rep_pen, ngram, early_stopping, st["run_seq"], st["run_score"], st["fin_seq"],
                        st["fin_score"], st["fin_flag"], st["fin_len"], st["unsat"])
        gap = min(gap, out["gap"])
        src = np.repeat(np.arange(B) * K, K) + out["parent"]
        for c in caches:
            c["k"], c["v"] = c["k"][src], c["v"][src]
        st = {k: out[k] for k in st}
        if not running(out["flags"], early_stopping):
            break
    n = 1 + int(st["fin_len"][::K].max())
    return st["fin_seq"][::K, :n].copy(), gap


def random_state(rng, B, K, V, cur_len, max_length, bos, pad, finished=0.0):
    """a plausible mid-search state: random histories, running scores sorted per item, some finished hypotheses"""
    R = B * K
    run_seq = np.full((R, max_length), pad, np.int64)
    run_seq[:, 0] = bos
    run_seq[:, 1:cur_len] = rng.integers(0, V - 3, size=(R, cur_len - 1))
    run_seq[:, 1:cur_len:3] = run_seq[:, 1:2]      # repeats, so that the penalty and the n-gram ban have work
    run_score = (-np.sort(rng.uniform(0.5, 3.0, size=(B, K)), axis=1) * cur_len).astype(np.float32).reshape(R)      # best beam first
    if cur_len == 1:
        run_score = np.tile(np.array([0.0] + [-1e9] * (K - 1), np.float32), B)
    fin_seq = np.full((R, max_length), pad, np.int64)
    fin_seq[:, 0] = bos
    fin_score = np.full(R, -1e9, np.float32)
    fin_flag = np.zeros(R, np.int32)
    fin_len = np.zeros(R, np.int32)
    for r in range(R):
        if cur_len > 2 and rng.uniform() < finished:
            n = int(rng.integers(1, cur_len))
            fin_seq[r, 1:n + 1] = rng.integers(0, V - 3, size=n)
            fin_score[r] = np.float32(-rng.uniform(1.0, 4.0))
            fin_flag[r], fin_len[r] = 1, n
    for b in range(B):      # finished slots sorted by score, as the merge leaves them
        o = np.argsort(-fin_score[b * K:(b + 1) * K], kind="stable") + b * K
        fin_seq[b * K:(b + 1) * K], fin_score[b * K:(b + 1) * K] = fin_seq[o], fin_score[o]
        fin_flag[b * K:(b + 1) * K], fin_len[b * K:(b + 1) * K] = fin_flag[o], fin_len[o]
    return run_seq, run_score, fin_seq, fin_score, fin_flag, fin_len
