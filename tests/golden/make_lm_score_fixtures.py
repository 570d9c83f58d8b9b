"""Golden fixtures of teacher-forced LM scoring (log-prob, loss and rank of given semantic tokens at every position).

The yardstick is the PREFIX evaluation of the reference's Roformer.forward (text2semantic/roformer/roformer.py:138-176 over HF transformers
RoFormerForCausalLM): the logits at position t are forward(semantic[:, :t + 1], use_cache=False).logits[:, -1] -- what generate() itself
computes at step t.  The reference's ONE-CALL forward over the whole sequence is not: on the installed transformers (5.x) it applies no causal
mask in the decoder's self-attention, so every position sees the future tokens (the same kind of artefact of running the unpinned reference
on a newer library as the cache aliasing documented in make_fixtures.roformer_fixtures).  This recipe asserts both facts:
  * the prefix logits of roformer.npz's greedy tokens reproduce its recorded per-step greedy_logits within 2e-6 of abs-max;
  * the one-call logits of the same tokens do not (they differ by more than 1e-2 of abs-max).

Model, seeded weights and inputs are make_fixtures.roformer_fixtures' (phone mode, the reference's flash-attention wrapper off).

  lm_score.npz, all cases B = 2 (<c> = a, b, c):
    <c>_semantic [B,T] int64 (BOS first), <c>_labels [B,T] int64, <c>_sem_len [B], <c>_enc_len [B] (c only, with ragged_mask)
    <c>_lp [B,T-1] float64   logit_y - logsumexp(logits), y = labels[:, t + 1], from the fp32 prefix logits in float64; 0 where not counted
    <c>_rank [B,T-1] int32   #{v: logit_v > logit_y} + #{v < y: logit_v == logit_y}; -1 where not counted
    <c>_rank_lo / <c>_rank_hi [B,T-1] int32   #{v: logit_v > logit_y + eps} and #{v: logit_v >= logit_y - eps} - 1 with
                             eps = 2 * 2e-5 * absmax: the ranks an implementation within the LM's logits bound (relmax 2e-5) can report
    <c>_loss float64         -(sum of the counted lp) / n_counted;  <c>_absmax float64;  <c>_n_counted int64
    b_logits_row0 [T,V] float32   case b's full prefix logits of batch row 0 (fp32 logits barely compress: both rows, 1.08 MB, would not
                             fit a committed file; row 1 is held through its lp, rank and rank bands like the other cases)
  Cases: (a) roformer.npz's greedy tokens (T 24; ranks near 0: the top-5 path); (b) random tokens, T 33, default_rng(11) (ranks spread over
  the vocabulary); (c) ragged: encoder lengths 23 / 15 under ragged_mask, semantic lengths 33 / 20, -100 labels inside the shorter row and,
  like the reference's collate, at and beyond every row's length.

  python tests/golden/make_lm_score_fixtures.py            # writes tests/golden/lm_score.npz
  python tests/golden/make_lm_score_fixtures.py --check    # regenerates into a temporary directory and compares array by array
"""
import argparse
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_fixtures as mf  # noqa: E402  (sets sys.path to the reference only)
import make_lm_beam_fixtures as mb  # noqa: E402  (build_model: roformer_fixtures' model, weights and inputs)

np, torch = mf.np, mf.torch
LOGITS_BOUND = 2e-5      # the project's LM logits bound (relmax, tests/test_gpu_frontend.py)
IGNORE = -100


def prefix_logits(m, phone, tone, spk, semantic, sem_len, mask=None):
    """[B,T,V] fp32: position t from a forward call over semantic[:, :t + 1]; rows at and beyond a sequence's length stay 0"""
    B, T = semantic.shape
    out = None
    kw = dict(encoder_attention_mask=None if mask is None else mf.tt(mask), spk_id=mf.tt(spk), use_cache=False)
    with torch.no_grad():
        for t in range(T):
            sem = np.where(np.arange(t + 1)[None, :] < sem_len[:, None], semantic[:, : t + 1], 0)      # (padding ids are never counted)
            lg = m(mf.tt(phone), mf.tt(tone), mf.tt(sem), **kw).logits[:, -1].numpy()
            if out is None:
                out = np.zeros((B, T, lg.shape[-1]), dtype=np.float32)
            out[:, t] = np.where((t < sem_len)[:, None], lg, 0)
    return out


def statistics(logits, labels, sem_len):
    """the recorded quantities of one case from its fp32 logits, in float64"""
    B, T, V = logits.shape
    absmax = float(np.abs(logits).max())
    eps = 2 * LOGITS_BOUND * absmax
    lp = np.zeros((B, T - 1))
    rank, lo, hi = (np.full((B, T - 1), -1, dtype=np.int32) for _ in range(3))
    for b in range(B):
        for t in range(T - 1):
            y = int(labels[b, t + 1])
            if t + 1 >= sem_len[b] or y == IGNORE:
                continue
            row = logits[b, t].astype(np.float64)
            mx = row.max()
            lp[b, t] = row[y] - (mx + np.log(np.exp(row - mx).sum()))
            rank[b, t] = int((row > row[y]).sum() + (row[:y] == row[y]).sum())
            lo[b, t] = int((row > row[y] + eps).sum())
            hi[b, t] = int((row >= row[y] - eps).sum()) - 1
    n = int((rank >= 0).sum())
    return dict(lp=lp, rank=rank, rank_lo=lo, rank_hi=hi, loss=np.float64(-lp.sum() / n), absmax=np.float64(absmax), n_counted=np.int64(n))


def make(out_dir):
    import transformers
    m, cfg, phone, tone, spk = mb.build_model()
    old = np.load(os.path.join(HERE, "roformer.npz"))
    V, bos = cfg["sem_vocab"], cfg["sem_bos"]
    out = {"transformers_version": np.frombuffer(transformers.__version__.encode(), dtype=np.uint8), "ragged_mask": old["ragged_mask"]}

    # (a) the greedy tokens; the two facts of the docstring
    sem_a = old["greedy_tokens"].astype(np.int64)
    full = np.array([sem_a.shape[1]] * 2)
    lg_a = prefix_logits(m, phone, tone, spk, sem_a, full)
    rec = old["greedy_logits"].transpose(1, 0, 2)                                # [steps,B,V] -> [B,steps,V]
    scale = float(np.abs(rec).max())
    e_prefix = float(np.abs(lg_a[:, : rec.shape[1]] - rec).max() / scale)
    with torch.no_grad():
        one = m(mf.tt(phone), mf.tt(tone), mf.tt(sem_a), spk_id=mf.tt(spk), use_cache=False, labels=mf.tt(sem_a))
    e_one = float(np.abs(one.logits.numpy()[:, : rec.shape[1]] - rec).max() / scale)
    print(f"prefix evaluation vs recorded step logits: {e_prefix:.2e} of abs-max; one-call forward: {e_one:.2e} (its loss {float(one.loss):.3f})")
    assert e_prefix < 2e-6, e_prefix
    assert e_one > 1e-2, f"the one-call forward now matches the step logits ({e_one:.2e}): the non-causal trap is gone, revisit the docstring"

    # (b) random tokens, (c) ragged
    rng = np.random.default_rng(11)
    T = 33
    sem_b = rng.integers(0, V - 3, size=(2, T)).astype(np.int64)
    sem_b[:, 0] = bos
    sem_c = rng.integers(0, V - 3, size=(2, T)).astype(np.int64)
    sem_c[:, 0] = bos
    len_c = np.array([33, 20])
    sem_c = np.where(np.arange(T)[None, :] < len_c[:, None], sem_c, IGNORE)      # the collate's padding value
    lab_c = sem_c.copy()
    lab_c[1, [5, 6, 12]] = IGNORE
    enc_len_c = old["ragged_len"].astype(np.int64)
    lg_b = prefix_logits(m, phone, tone, spk, sem_b, np.array([T, T]))
    lg_c = prefix_logits(m, phone, tone, spk, sem_c, len_c, mask=old["ragged_mask"])

    for tag, sem, lab, sl, lg in (("a", sem_a, sem_a, full, lg_a), ("b", sem_b, sem_b, np.array([T, T]), lg_b), ("c", sem_c, lab_c, len_c, lg_c)):
        st = statistics(lg, lab, sl)
        out[tag + "_semantic"], out[tag + "_labels"], out[tag + "_sem_len"] = sem, lab, sl.astype(np.int64)
        for k, v in st.items():
            out[f"{tag}_{k}"] = v
        r, pinned = st["rank"][st["rank"] >= 0], int(((st["rank_lo"] == st["rank_hi"]) & (st["rank"] >= 0)).sum())
        print(f"case {tag}: T {sem.shape[1]}, counted {st['n_counted']}, loss {st['loss']:.4f}, abs-max {st['absmax']:.2f}, ranks {r.min()} .. {r.max()} "
              f"(median {int(np.median(r))}), pinned exactly {pinned}, widest band {int((st['rank_hi'] - st['rank_lo']).max())}")
        assert 2 * pinned >= st["n_counted"], f"case {tag}: fewer than half of the ranks are pinned"
    out["c_enc_len"] = enc_len_c
    assert (out["a_rank_lo"] == out["a_rank_hi"]).all()
    out["b_logits_row0"] = lg_b[0].copy()
    np.savez_compressed(os.path.join(out_dir, "lm_score.npz"), **out)
    print("lm_score.npz:", os.path.getsize(os.path.join(out_dir, "lm_score.npz")), "bytes")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="regenerate into a temporary directory and compare with the committed file")
    a = ap.parse_args()
    if not a.check:
        make(HERE)
        return
    with tempfile.TemporaryDirectory() as d:
        new = make(d)
        old = np.load(os.path.join(HERE, "lm_score.npz"))
        assert set(old.files) == set(new), (sorted(old.files), sorted(new))
        bad = [k for k in new if not (old[k].dtype == np.asarray(new[k]).dtype and np.array_equal(old[k], new[k]))]
        assert not bad, f"regenerated arrays differ: {bad}"
    print("lm_score.npz reproduced")


if __name__ == "__main__":
    main()
