"""Golden fixtures of the Llama's teacher-forced scoring: the reference's own `Llama.forward` (text2semantic/llama/llama.py:73-117, imported
from the reference by path through make_llama_fixtures.build_model, never copied) on the installed transformers, with the toy config and the
committed weight seed of llama.npz.  Unlike the RoFormer's one-call forward this one is causal: its logits at the
semantic positions equal the per-step logits that `generate` recorded in llama.npz (asserted below, 2e-6 of abs-max), and its `.loss` is the
plain mean of -log_softmax over the full vocabulary at the shifted labels (asserted), so `forward` is the oracle for logits, loss and ranks.

  llama_score.npz   per case and row (B = 1 through forward(phone, tone, semantic, labels = input_ids), the reference's own stream
                    [108, phones, 109, 108 + K, semantic + 108, EOS], llama.py:98-101)
                      <case>_r<b>_semantic   the semantic tokens (generate's numbering): "greedy" = llama.npz's recorded greedy tokens,
                                             "random" = 30 seeded random tokens
                      <case>_r<b>_ids        the stream the reference built (checked against its own input_ids)
                      <case>_r<b>_logits     forward's logits [S, vocab], fp32
                      <case>_r<b>_loss       forward's .loss (labels = input_ids: every position of the stream but the last is counted)
                      <case>_r<b>_lp, _rank  per position t (0 .. S - 2): log_softmax(logits[t])[ids[t + 1]] in float64, and the number of
                                             columns above the label's logit, ties to the lowest index
                    "batch": the two "random" rows as one right-padded batch through input_ids= / attention_mask= with labels -100 on the padding
                    and on a few positions inside the shorter row
                      batch_ids, batch_mask, batch_labels [2, S], batch_loss (pooled over both rows), batch_n (counted positions)
                    weight_seed, random_seed, transformers_version

Assertions of the maker: the batched rows' logits equal the B = 1 rows' within 1e-5; the one-call logits equal llama.npz's step logits within
2e-6 of abs-max; the loss equals the mean of -lp; in every case at least 90 % of the counted positions are pinned -- no other reference logit
within eps = 2 * 2e-5 * absmax(logits) of the label's -- so a test may demand the rank there.

  python tests/golden/make_llama_score_fixtures.py            # writes tests/golden/llama_score.npz
  python tests/golden/make_llama_score_fixtures.py --check    # regenerates into a temporary directory and compares array by array
"""
import argparse
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_llama_fixtures as ml  # noqa: E402  (sets sys.path to the reference only)

np, torch, mf = ml.np, ml.torch, ml.mf
LOGITS_TOL = 2e-5
RANDOM_SEED = 7
N_RANDOM = 30
HOLES = (20, 21, 33)      # positions inside the shorter row of the batch whose labels are -100


def stats(logits, labels):
    """per position t: (log_softmax(logits[t])[labels[t + 1]] in float64, rank with ties to the lowest index, counted, pinned)"""
    S = logits.shape[0]
    eps = 2 * LOGITS_TOL * float(np.abs(logits).max())
    lp, rank, counted, pinned = np.zeros(S - 1, np.float64), np.full(S - 1, -1, np.int32), np.zeros(S - 1, bool), np.zeros(S - 1, bool)
    for t in range(S - 1):
        y = int(labels[t + 1])
        if y < 0:
            continue
        row = logits[t].astype(np.float64)
        m = row.max()
        lp[t] = row[y] - (m + np.log(np.exp(row - m).sum()))
        rank[t] = int((row > row[y]).sum() + (row[:y] == row[y]).sum())
        counted[t] = True
        pinned[t] = np.abs(np.delete(row, y) - row[y]).min() > eps
    return lp, rank, counted, pinned


def one_row(m, cfg, phone, semantic):
    """the reference's forward(phone, tone, semantic, labels = input_ids) for one row -> (ids [S], logits [S, vocab], loss)"""
    ids = np.concatenate([[cfg["text_bos"]], phone, [cfg["text_eos"]], [cfg["bos"]], semantic + cfg["shift"], [cfg["eos"]]]).astype(np.int64)
    seen = []
    hook = m.llama.register_forward_pre_hook(lambda _m, _a, kw: seen.append(kw["input_ids"].numpy().copy()), with_kwargs=True)
    try:
        with torch.no_grad():
            ph = mf.tt(phone[None])
            out = m(ph, torch.ones_like(ph), mf.tt(semantic[None].copy()), labels=mf.tt(ids[None]))      # (forward shifts `semantic` in place)
    finally:
        hook.remove()
    assert len(seen) == 1 and np.array_equal(seen[0][0], ids), "the reference built another stream"
    return ids, out.logits[0].float().numpy().copy(), float(out.loss)


def make(out_dir):
    import transformers
    old = np.load(os.path.join(HERE, "llama.npz"))
    weight_seed = int(old["weight_seed"])
    m, cfg = ml.build_model(weight_seed)
    phones = ml.phones()
    assert all(np.array_equal(phones[b], old[f"phone_r{b}"]) for b in range(2))
    rng = np.random.RandomState(RANDOM_SEED)
    out = {}
    rows = {}
    for case in ("greedy", "random"):
        for b in range(2):
            sem = old[f"greedy_r{b}_tokens"].astype(np.int64) if case == "greedy" else rng.randint(0, ml.K, N_RANDOM).astype(np.int64)
            assert sem.max() < ml.K      # (no EOS inside: forward appends it)
            ids, logits, loss = one_row(m, cfg, phones[b], sem)
            lp, rank, counted, pinned = stats(logits, ids)
            assert counted.all() and abs(loss - float(-lp.mean())) < 1e-5, (loss, -lp.mean())
            share = pinned.sum() / counted.sum()
            print(f"  {case} r{b}: S {len(ids)}, loss {loss:.5f} (mean of -lp {-lp.mean():.5f}), pinned {pinned.sum()}/{counted.sum()}, "
                  f"logit absmax {np.abs(logits).max():.3f}")
            assert share >= 0.9, share
            if case == "greedy":      # the one-call forward is the cached decode: llama.npz's recorded step logits of the columns 108 ..
                ref = old[f"greedy_r{b}_logits"]
                at = len(phones[b]) + 2
                got = logits[at:at + len(ref), cfg["shift"]:]
                rel = float(np.abs(got - ref).max() / np.abs(ref).max())
                print(f"    one call against the recorded steps: relmax {rel:.2e}")
                assert rel < 2e-6, rel
            p = f"{case}_r{b}_"
            out[p + "semantic"], out[p + "ids"], out[p + "logits"] = sem, ids, logits.astype(np.float32)
            out[p + "loss"], out[p + "lp"], out[p + "rank"] = np.float64(loss), lp, rank
            rows[(case, b)] = (ids, logits)
    # the two random rows as one right-padded batch through input_ids= / attention_mask=
    r0, r1 = rows[("random", 0)], rows[("random", 1)]
    S = max(len(r0[0]), len(r1[0]))
    ids = np.full((2, S), cfg["pad"], dtype=np.int64)
    mask = np.zeros((2, S), dtype=np.int64)
    for b, (i, _) in enumerate((r0, r1)):
        ids[b, :len(i)] = i
        mask[b, :len(i)] = 1
    short = int(np.argmin(mask.sum(1)))
    labels = np.where(mask == 1, ids, -100)
    labels[short, list(HOLES)] = -100
    assert mask[short].sum() > max(HOLES) and mask.sum(1).min() < S
    with torch.no_grad():
        o = m(None, None, None, input_ids=mf.tt(ids), attention_mask=mf.tt(mask), labels=mf.tt(labels))
    bl = o.logits.float().numpy()
    tot, n, pin = 0.0, 0, 0
    for b, (i, lg) in enumerate((r0, r1)):
        d = float(np.abs(bl[b, :len(i)] - lg).max())
        print(f"  batch row {b}: max |batched - alone| {d:.2e}")
        assert d < 1e-5, d
        lp, _, counted, pinned = stats(bl[b], labels[b])
        tot, n, pin = tot - lp.sum(), n + int(counted.sum()), pin + int((pinned & counted).sum())
    print(f"  batch: pooled loss {float(o.loss):.5f} (restated {tot / n:.5f}) over {n} positions, pinned {pin}/{n}")
    assert abs(float(o.loss) - tot / n) < 1e-5 and pin >= 0.9 * n
    out.update(batch_ids=ids, batch_mask=mask, batch_labels=labels, batch_loss=np.float64(float(o.loss)), batch_n=np.int64(n),
               weight_seed=np.int64(weight_seed), random_seed=np.int64(RANDOM_SEED),
               transformers_version=np.frombuffer(transformers.__version__.encode(), dtype=np.uint8))
    np.savez_compressed(os.path.join(out_dir, "llama_score.npz"), **out)
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
        old = np.load(os.path.join(HERE, "llama_score.npz"))
        assert set(old.files) == set(new), (sorted(old.files), sorted(new))
        bad = [k for k in new if not (old[k].dtype == np.asarray(new[k]).dtype and np.array_equal(old[k], new[k]))]
        assert not bad, f"regenerated arrays differ: {bad}"
    print("llama_score.npz reproduced")


if __name__ == "__main__":
    main()
