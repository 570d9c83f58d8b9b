"""numpy restatement of the Llama's greedy beam search (lds_llama_generate_beam; transformers generation/utils.py _beam_search as the reference's
Llama.generate drives it, length_penalty 1): one step in the state layout of lds_test_llama_beam_step (include/lds_test.h), and a whole decode
over tests/llama_numpy.py's cached decoder.  What differs from tests/lm_beam_numpy.py's step: every item continues a decoder prompt of its own
length (cur_len = prompt_len[b] + step; the finished score divides by cur_len + 1 - prompt_len[b], the heuristic by that or by max_length -
prompt_len[b]), log_softmax runs over the whole vocabulary and the ids below first_free_id get -inf after the repetition penalty and the
n-gram ban, and an item whose own loop has ended is frozen.  Storage fp32, the decoder's sums float64, as in llama_numpy."""
import numpy as np

import llama_numpy as LN
import lm_beam_numpy as NB

MASK, ZERO = NB.MASK, NB.ZERO


def item_running(unsat, all_fin, all_hit, early_stopping):
    """_beam_search_has_unfinished_sequences for ONE item"""
    return bool(unsat) and (early_stopping != 1 or not all_fin) and not all_hit


def beam_step(logits, K, step, max_length, eos, rep_pen, ngram, early_stopping, first_free, prompt_len, ended, run_seq, run_score, fin_seq,
              fin_score, fin_flag, fin_len, unsat):
    """one step; early_stopping 1 = True, 0 = False, 2 = "never".  logits [B*K, V] over the whole vocabulary; prompt_len, ended [B]; the other
    arrays as lm_beam_numpy.beam_step, fin_len counting generated tokens.  Returns the new state (an ended item's unchanged, its parents 0 ..
    K - 1), "ended" [B] after the step, "flags" (lm_beam_numpy's bits over the items that ran, plus 16 = some item still runs) and "gap", the
    smallest score gap at a selection of the step."""
    R, V = logits.shape
    B = R // K
    out = dict(run_seq=run_seq.copy(), run_score=run_score.astype(np.float32).copy(), fin_seq=fin_seq.copy(), fin_score=fin_score.astype(np.float32).copy(),
               fin_flag=fin_flag.copy(), fin_len=fin_len.copy(), unsat=unsat.copy(), parent=np.tile(np.arange(K, dtype=np.int32), B),
               ended=np.asarray(ended).astype(np.int32).copy())
    bits, gap = 0, np.inf
    for b in range(B):
        if ended[b]:
            out["ended"][b] = 2      # frozen and copied through: the kernel's "both buffers hold it"
            continue
        rows = slice(b * K, (b + 1) * K)
        pl = int(prompt_len[b])
        cur_len = pl + step
        gen = cur_len + 1 - pl
        lp = NB.log_softmax(logits[rows])
        for k in range(K):
            hist = run_seq[b * K + k, :cur_len]
            if rep_pen != 1.0:
                for t in set(int(t) for t in hist):
                    if 0 <= t < V:
                        lp[k, t] = lp[k, t] * np.float32(rep_pen) if lp[k, t] < 0 else lp[k, t] / np.float32(rep_pen)
            for t in NB.ngram_banned(hist, ngram):
                if 0 <= t < V:
                    lp[k, t] = -np.inf
            lp[k, :first_free] = -np.inf
        flat = (lp + run_score[rows].astype(np.float32)[:, None]).astype(np.float32).reshape(-1)
        sel = NB._top(flat, 2 * K)
        gap = min(gap, NB._gap(flat, [2 * K, K]))
        topv, topb, topt = flat[sel], sel // V, sel % V
        hit = (topt == eos) | (cur_len + 1 >= max_length)
        trl = np.array([topv[j] + (MASK if hit[j] else ZERO) for j in range(2 * K)], np.float32)
        run_j = NB._top(trl, K)
        all_fin = bool(fin_flag[rows].all())
        f = np.zeros(2 * K, np.float32)
        for j in range(2 * K):
            did = bool(hit[j]) and j < K
            v = np.float32(topv[j] / np.float32(gen))
            v = np.float32(v + (MASK if (all_fin and early_stopping == 1) else ZERO))
            v = np.float32(v + (ZERO if unsat[b] else MASK))
            v = np.float32(v + (ZERO if did else MASK))
            f[j] = v
        ms = np.concatenate([fin_score[rows].astype(np.float32), f])
        fin_j = NB._top(ms, K)
        gap = min(gap, NB._gap(trl, [K]), NB._gap(ms, [K, 1]))
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
                out["fin_seq"][r, :cur_len + 1] = fin_seq[src, :cur_len + 1]
                out["fin_score"][r], out["fin_flag"][r], out["fin_len"][r] = fin_score[src], fin_flag[src], fin_len[src]
            else:
                jj = m - K
                out["fin_seq"][r, :cur_len] = run_seq[b * K + topb[jj], :cur_len]
                out["fin_seq"][r, cur_len] = topt[jj]
                out["fin_score"][r], out["fin_flag"][r], out["fin_len"][r] = ms[m], int(hit[jj] and jj < K), gen
        hyp = max_length - pl if early_stopping == 2 else gen
        best = np.float32(out["run_score"][b * K] / np.float32(hyp))
        worst = out["fin_score"][rows].min()
        improve = any(best > (worst if out["fin_flag"][b * K + k] else MASK) for k in range(K))
        out["unsat"][b] = int(bool(unsat[b]) and improve)
        nall_fin, all_hit = bool(out["fin_flag"][rows].all()), bool(hit.all())
        run = item_running(out["unsat"][b], nall_fin, all_hit, early_stopping)
        out["ended"][b] = 0 if run else 1
        bits |= (1 if out["unsat"][b] else 0) | (0 if nall_fin else 2) | (0 if all_hit else 4) | (16 if run else 0)
    out["flags"] = bits
    out["gap"] = gap
    return out


def _clone(dec):
    """a decoder that continues from dec's cache (the arrays are never written again, so the lists' copies may share them)"""
    new = LN.Decoder.__new__(LN.Decoder)
    new.__dict__.update(dec.__dict__)
    new.k, new.v = [list(x) for x in dec.k], [list(x) for x in dec.v]
    return new


def generate_beam(w, cfg, inv_freq, ids, K, max_length, rep_pen=1.0, ngram=0, early_stopping=1):
    """one row: ids = the prompt (model ids: llama_numpy.prompt_ids, possibly followed by a semantic prompt).  The prompt's positions but the
    last run once; the K beams continue from copies of that cache, reordered by parent after every step (HF's reorder_cache).  Returns
    (ids [n]: the prompt and the best finished hypothesis, EOS kept; the smallest decision margin of the run; the number of steps run)."""
    ids = [int(t) for t in ids]
    pl = len(ids)
    if pl >= max_length:
        raise ValueError(f"the prompt has {pl} ids, max_length is {max_length}")
    dec = LN.Decoder(w, cfg, inv_freq)
    dec.head = np.ascontiguousarray(w["llama.lm_head.weight"])      # the whole vocabulary: HF's log_softmax sees the banned columns
    for t in ids[:-1]:
        dec.step(t, want_logits=False)
    decs = [_clone(dec) for _ in range(K)]
    run_seq = np.full((K, max_length), cfg["pad"], np.int64)
    run_seq[:, :pl] = ids
    st = dict(run_seq=run_seq, run_score=np.array([0.0] + [-1e9] * (K - 1), np.float32), fin_seq=run_seq.copy(), fin_score=np.full(K, -1e9, np.float32),
              fin_flag=np.zeros(K, np.int32), fin_len=np.zeros(K, np.int32), unsat=np.ones(1, np.int32))
    gap, steps = np.inf, 0
    for step in range(max_length - pl):
        lg = np.stack([d.step(st["run_seq"][k, pl - 1 + step]) for k, d in enumerate(decs)])
        out = beam_step(lg, K, step, max_length, cfg["eos"], rep_pen, ngram, early_stopping, cfg["shift"], [pl], [0], st["run_seq"], st["run_score"],
                        st["fin_seq"], st["fin_score"], st["fin_flag"], st["fin_len"], st["unsat"])
        gap = min(gap, out["gap"])
        decs = [_clone(decs[int(p)]) for p in out["parent"]]
        st = {k: out[k] for k in st}
        steps = step + 1
        if out["ended"][0]:
            break
    n = pl + int(st["fin_len"][0])
    return st["fin_seq"][0, :n].copy(), gap, steps


def random_state(rng, B, K, V, step, max_length, first_free, pad, prompt_len, finished=0.0):
    """a plausible mid-search state at `step` for items with the given prompt lengths: histories of phone ids then free ids, running scores
    sorted per item, some finished hypotheses (fin_len = generated tokens); layout of lm_beam_numpy.random_state"""
    R = B * K
    run_seq = np.full((R, max_length), pad, np.int64)
    fin_seq = np.full((R, max_length), pad, np.int64)
    fin_score = np.full(R, -1e9, np.float32)
    fin_flag = np.zeros(R, np.int32)
    fin_len = np.zeros(R, np.int32)
    run_score = np.zeros(R, np.float32)
    for b in range(B):
        pl = int(prompt_len[b])
        cur = min(pl + step, max_length - 1)
        prompt = rng.integers(0, max(first_free, 1), size=pl)
        rows = slice(b * K, (b + 1) * K)
        run_seq[rows, :pl] = prompt
        fin_seq[rows, :pl] = prompt
        run_seq[rows, pl:cur] = rng.integers(first_free, V - 3, size=(K, cur - pl))
        run_seq[rows, pl + 1:cur:3] = run_seq[rows, pl:pl + 1] if cur > pl else 0      # repeats, so that the penalty and the n-gram ban have work
        run_score[rows] = (-np.sort(rng.uniform(0.5, 3.0, size=K)) * max(step, 1)).astype(np.float32)
        if step == 0:
            run_score[rows] = np.array([0.0] + [-1e9] * (K - 1), np.float32)
        for r in range(b * K, (b + 1) * K):
            if step > 1 and rng.uniform() < finished:
                n = int(rng.integers(1, step + 1))
                fin_seq[r, pl:pl + n] = rng.integers(first_free, V - 3, size=n)
                fin_score[r] = np.float32(-rng.uniform(1.0, 4.0))
                fin_flag[r], fin_len[r] = 1, n
        o = np.argsort(-fin_score[rows], kind="stable") + b * K
        fin_seq[rows], fin_score[rows], fin_flag[rows], fin_len[rows] = fin_seq[o], fin_score[o], fin_flag[o], fin_len[o]
    return run_seq, run_score, fin_seq, fin_score, fin_flag, fin_len
