"""Golden fixtures of the LM decode modes beyond greedy / sampling: greedy beam search and no-repeat n-gram blocking.

Runs the reference's Roformer.generate (text2semantic/roformer/roformer.py over HF transformers GenerationMixin) on the same seeded
weights and inputs as make_fixtures.py's roformer.npz, which it imports for its import hygiene (only the reference is importable by
package name), weights and inputs.  make_fixtures.py itself is not changed.

  roformer_beam.npz   <case>_tokens for every case below, <case>_margin (the smallest score gap at any selection made during the run:
                      top-k / argmax neighbours, and the distance of a sampling uniform from the CDF steps), the EOS bias, the ragged
                      lengths / mask, the sampled case's uniforms and the transformers version.

Every case must exercise its feature (beams differ from greedy, the n-gram ban changes a token, an early EOS is followed by PAD) and
have a margin of at least 1e-3, so that no recorded token rests on a tie or on the last bits of a float sum.

  python tests/golden/make_lm_beam_fixtures.py            # writes tests/golden/roformer_beam.npz
  python tests/golden/make_lm_beam_fixtures.py --check    # regenerates into a temporary directory and compares array by array
"""
import argparse
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_fixtures as mf  # noqa: E402  (sets sys.path to the reference only)

np, torch = mf.np, mf.torch
MIN_MARGIN = 1e-3
MASKED = -5e8      # scores carrying one of HF's -1e9 masks: their order among themselves never reaches the output
TOPK = torch.topk

# (tag, generate keywords); EOS_BIAS is added to the LM head's EOS bias for the "eos" case
EOS_BIAS = 14.0
CASES = [
    ("beam4", dict(num_beams=4, max_length=24)),
    ("beam4_ngram3", dict(num_beams=4, max_length=24, no_repeat_ngram_size=3, repetition_penalty=1.2)),
    ("beam4_eos", dict(num_beams=4, max_length=40)),
    ("beam3_ragged", dict(num_beams=3, max_length=24)),
    ("greedy_ngram2", dict(num_beams=1, max_length=24, no_repeat_ngram_size=2)),
    ("sample_ngram2", dict(num_beams=1, max_length=40, no_repeat_ngram_size=2, do_sample=True)),
]


class Margins:
    """the smallest score gap at a selection that reaches the returned tokens, over every torch.topk / torch.argmax call of a run:
      greedy argmax: best vs second; sampling top-k: ranks k | k + 1;
      beam search (K beams) -- top 2K of the K * V continuations: ranks 2K | 2K + 1 (which candidates exist) and K | K + 1 (which of
      them may finish); next running beams, K of 2K: rank K | K + 1; finished merge, K of 3K: ranks K | K + 1 and 1 | 2 (the output);
      and the distance of every sampling uniform from the CDF steps.  Scores carrying one of HF's -1e9 masks are left out."""

    def __init__(self, K):
        self.K, self.gap, self.drawn = K, float("inf"), []

    def note(self, scores, k):
        s = scores.detach().float().reshape(-1, scores.shape[-1])
        K, w = self.K, s.shape[-1]
        ranks = [k] if K == 1 else [K] if w == 2 * K else [K, 1] if w == 3 * K else [2 * K, K]
        top = TOPK(s, min(max(ranks) + 1, w), dim=-1).values
        for row in top:
            for r in ranks:
                if r < row.numel() and bool(row[r] > MASKED) and bool(torch.isfinite(row[r - 1])):
                    self.gap = min(self.gap, float(row[r - 1] - row[r]))

    def note_draw(self, cdf, u):
        self.gap = min(self.gap, float((cdf - u[:, None]).abs().min()))


def build_model():
    """make_fixtures.roformer_fixtures' model, weights and inputs"""
    import yaml
    from text2semantic.roformer import roformer as ref_lm
    args = yaml.safe_load(open(os.path.join(mf.REF, "configs", "config.yaml")))
    t2s = args["text2semantic"]
    t2s["model"]["mode"] = "phone"
    t2s["model"]["codebook_path"] = "/nonexistent"
    t2s["train"]["use_flash_attn"] = False
    cfg = mf.arch.roformer_config(n_spk=args["common"]["n_spk"], semantic_kmeans_num=t2s["model"]["semantic_kmeans_num"])
    m = ref_lm.get_model(args["common"]["n_spk"], **t2s).eval()
    state = mf.arch.roformer_init_state(cfg, mf.SEED_W, mf.init_weights)
    m.load_state_dict({k: mf.tt(v) for k, v in state.items()}, strict=True)
    B, L = 2, 23
    phone = (np.arange(B * L).reshape(B, L) * 7 % 107 + 1).astype(np.int64)
    tone = (np.arange(B * L).reshape(B, L) * 5 % 12).astype(np.int64)
    spk = np.stack([np.full(L, 3), np.full(L, 200)]).astype(np.int64)
    return m, cfg, phone, tone, spk


def run(m, cfg, phone, tone, spk, kw, mask=None, eos_bias=None):
    """one reference generate call under the margin hooks (use_cache=False: see make_fixtures.roformer_fixtures)"""
    mg = Margins(kw.get("num_beams", 1))
    real = (torch.topk, torch.argmax, torch.multinomial)

    def topk(x, k, *a, **k2):
        mg.note(x, k)
        return real[0](x, k, *a, **k2)

    def argmax(x, *a, **k2):
        mg.note(x, 1)
        return real[1](x, *a, **k2)

    def inverse_cdf_multinomial(probs, num_samples, **_k):      # make_fixtures' reproducible draw
        assert num_samples == 1
        u = torch.rand(probs.shape[0])
        c = probs.float().cumsum(-1)
        mg.note_draw(c, u)
        mg.drawn.append(u.numpy().copy())
        return torch.searchsorted(c, u[:, None].contiguous(), right=True).clamp(max=probs.shape[-1] - 1)

    args = dict(attention_mask=None if mask is None else mf.tt(mask), use_cache=False, do_sample=False, temperature=1.0, top_k=5, top_p=1.0,
                repetition_penalty=1.0, num_beams=1, no_repeat_ngram_size=0, early_stopping=True, spk_id=mf.tt(spk), end_gate_threshold=None)
    args.update(kw)
    if eos_bias is not None:
        m.semantic_decoder.cls.predictions.bias.data[cfg["sem_eos"]] += eos_bias
    torch.manual_seed(5)
    torch.topk, torch.argmax, torch.multinomial = topk, argmax, inverse_cdf_multinomial
    try:
        toks = m.generate(mf.tt(phone), mf.tt(tone), **args).numpy()
    finally:
        torch.topk, torch.argmax, torch.multinomial = real
        if eos_bias is not None:
            m.semantic_decoder.cls.predictions.bias.data[cfg["sem_eos"]] -= eos_bias
    return toks, mg.gap, mg.drawn


def make(out_dir):
    import transformers
    m, cfg, phone, tone, spk = build_model()
    eos, pad = cfg["sem_eos"], cfg["sem_pad"]
    L = phone.shape[1]
    lens = np.array([L, 15], dtype=np.int64)
    mask = (np.arange(L)[None, :] < lens[:, None]).astype(np.int64)
    out = {"transformers_version": np.frombuffer(transformers.__version__.encode(), dtype=np.uint8), "eos_bias": np.float32(EOS_BIAS),
           "ragged_len": lens, "ragged_mask": mask}
    plain = {}
    for tag, kw in CASES:
        extra = dict(mask=mask if "ragged" in tag else None, eos_bias=EOS_BIAS if "eos" in tag else None)
        toks, gap, drawn = run(m, cfg, phone, tone, spk, kw, **extra)
        # the same call without the feature under test (beams -> greedy, n-gram ban -> none)
        base_kw = dict(kw, num_beams=1) if kw.get("num_beams", 1) > 1 else dict(kw, no_repeat_ngram_size=0)
        base, _, _ = run(m, cfg, phone, tone, spk, base_kw, **extra)
        n = min(toks.shape[1], base.shape[1])
        changed = toks.shape != base.shape or not np.array_equal(toks[:, :n], base[:, :n])
        print(f"{tag}: tokens {toks.shape}, margin {gap:.3e}, differs from {'greedy' if 'beam' in tag else 'no ban'}: {changed}")
        print("   ", toks.tolist())
        assert gap >= MIN_MARGIN, f"{tag}: a selection rests on a score gap of {gap:.3e} < {MIN_MARGIN}"
        assert changed, f"{tag}: the feature does not change the output"
        if "beam" in tag:      # every row of a beam search differs from its greedy decode
            assert all(not np.array_equal(toks[b, :n], base[b, :n]) for b in range(toks.shape[0])), tag
        out[tag + "_tokens"] = toks
        out[tag + "_margin"] = np.float64(gap)
        if drawn:      # the sampler's uniforms [steps][B] (the library takes them in place of torch.multinomial's draw)
            out[tag + "_uniforms"] = np.stack(drawn)
        plain[tag] = base
    e = out["beam4_eos_tokens"]      # one row ends at an early EOS followed by PAD, the other runs to max_length
    ends = [int(np.argmax(r == eos)) if (r == eos).any() else None for r in e]
    assert e.shape[1] == 40 and any(x is None for x in ends) and any(x is not None and x + 1 < e.shape[1] for x in ends), ends
    for r, x in zip(e, ends):
        if x is not None:
            assert (r[x + 1:] == pad).all(), r
    np.savez_compressed(os.path.join(out_dir, "roformer_beam.npz"), **out)
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
        old = np.load(os.path.join(HERE, "roformer_beam.npz"))
        assert set(old.files) == set(new), (sorted(old.files), sorted(new))
        bad = [k for k in new if not (old[k].dtype == np.asarray(new[k]).dtype and np.array_equal(old[k], new[k]))]
        assert not bad, f"regenerated arrays differ: {bad}"
    print("roformer_beam.npz reproduced")


if __name__ == "__main__":
    main()
