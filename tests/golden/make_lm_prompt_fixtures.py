"""Golden fixtures of prompted LM generation: the decode continued from given semantic tokens.

The reference's Roformer.generate (text2semantic/roformer/roformer.py:179-244) calls HF's semantic_decoder.generate without a decoder
prompt; its **kwargs drop one.  HF's call takes it as input_ids=, so this recipe makes the reference model's own calls -- its text_encoder,
then semantic_decoder.generate with the GenerationConfig of roformer.py:220-233 -- and adds input_ids=prompt.  Weights, inputs, the margin
hooks and the reproducible inverse-CDF draw are make_fixtures.py's / make_lm_beam_fixtures.py's (imported, not changed); use_cache=False
and the flash wrapper off as there.

  lm_prompt.npz   per case: <case>_prompt [B,P], <case>_prompt_len [B], <case>_tokens (the prompt, then the generated ids; EOS kept, PAD
                  after it; cropped to the longest row), <case>_margin (the smallest score gap at any selection of the run, and the distance
                  of a sampling uniform from the CDF steps), <case>_uniforms [steps,B] where sampled; greedy_logits_row0 [steps,V];
                  cases_json (every case's generate keywords); eos_bias; ragged_len / ragged_mask; the transformers version.
                  The ragged case (prompt lengths 9 and 4, phone lengths 23 and 15) is recorded ROW BY ROW, each row alone at B = 1 with its
                  phones cropped -- HF has no right-padded form of a decoder prompt, and "row b equals row b alone" is the library's
                  definition: ragged_greedy_* and ragged_sample_* hold the rows assembled into one batch.

Every case has a margin of at least 1e-3 and exercises its feature (asserted below).

  python tests/golden/make_lm_prompt_fixtures.py            # writes tests/golden/lm_prompt.npz
  python tests/golden/make_lm_prompt_fixtures.py --check    # regenerates into a temporary directory and compares array by array
"""
import argparse
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_fixtures as mf  # noqa: E402  (sets sys.path to the reference only)
import make_lm_beam_fixtures as mb  # noqa: E402

np, torch = mf.np, mf.torch
MIN_MARGIN = mb.MIN_MARGIN
EOS_BIAS = mb.EOS_BIAS
P = 9
# prompts of the n-gram and the penalty case: the first 16 tokens of roformer.npz's greedy run, whose row 1 has fallen into a loop by then
# (it repeats one token); row 0 has not and rides along
NGRAM_P, PENALTY_P, LOOP_ROW = 16, 16, 1
RAGGED_SEED = 7      # torch seed of the ragged rows' draws: the first seed from 5 on whose draws all stay MIN_MARGIN away from a CDF step (5: 8.8e-4, 6: 1.5e-4)
CASES = {
    "greedy": dict(max_length=24),
    "sample": dict(max_length=40, do_sample=True, top_k=5, repetition_penalty=1.2),
    "ngram": dict(max_length=24, no_repeat_ngram_size=2),
    "penalty": dict(max_length=24, repetition_penalty=1.3),
    "eos": dict(max_length=40),
    "ragged_greedy": dict(max_length=24),
    "ragged_sample": dict(max_length=40, do_sample=True, top_k=5, repetition_penalty=1.2),
}
DEFAULTS = dict(do_sample=False, temperature=1.0, top_k=5, top_p=1.0, repetition_penalty=1.0, no_repeat_ngram_size=0)


def run(m, cfg, phone, tone, spk, prompt, kw, mask=None, eos_bias=None, seed=5):
    """one prompted generate of the reference model under the margin hooks -> (tokens, margin, uniforms drawn, per-step logits [steps,B,V])"""
    from transformers import GenerationConfig
    mg = mb.Margins(1)
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

    a = dict(DEFAULTS, **kw)
    logits = []
    hook = m.semantic_decoder.cls.register_forward_hook(lambda _m, _i, o: logits.append(o[:, -1].detach().numpy().copy()))
    am = None if mask is None else mf.tt(mask)
    if eos_bias is not None:
        m.semantic_decoder.cls.predictions.bias.data[cfg["sem_eos"]] += eos_bias
    torch.manual_seed(seed)
    torch.topk, torch.argmax, torch.multinomial = topk, argmax, inverse_cdf_multinomial
    try:
        emb = m.text_encoder.embeddings(mf.tt(phone), mf.tt(tone)) + m.spk_emb(mf.tt(spk))
        enc = m.text_encoder(inputs_embeds=emb, attention_mask=am, use_cache=False)[0]
        gc = GenerationConfig(max_length=a["max_length"], do_sample=a["do_sample"], temperature=a["temperature"], top_k=a["top_k"], top_p=a["top_p"],
                              repetition_penalty=a["repetition_penalty"], num_beams=1, no_repeat_ngram_size=a["no_repeat_ngram_size"], early_stopping=False,
                              bos_token_id=m.semantic_bos_token_id, eos_token_id=m.semantic_eos_token_id, pad_token_id=m.semantic_pad_token_id)
        toks = m.semantic_decoder.generate(input_ids=mf.tt(prompt), encoder_hidden_states=enc, encoder_attention_mask=am, attention_mask=None,
                                           use_cache=False, generation_config=gc, logits_processor=None).numpy()
    finally:
        torch.topk, torch.argmax, torch.multinomial = real
        hook.remove()
        if eos_bias is not None:
            m.semantic_decoder.cls.predictions.bias.data[cfg["sem_eos"]] -= eos_bias
    return toks, mg.gap, mg.drawn, np.stack(logits)


def random_prompt(cfg, B, n, seed):
    p = np.random.default_rng(seed).integers(0, cfg["semantic_kmeans_num"], size=(B, n)).astype(np.int64)
    p[:, 0] = cfg["sem_bos"]
    return p


def make(out_dir):
    import transformers
    m, cfg, phone, tone, spk = mb.build_model()
    eos, pad = cfg["sem_eos"], cfg["sem_pad"]
    B, L = phone.shape
    lens = np.array([L, 15], dtype=np.int64)
    mask = (np.arange(L)[None, :] < lens[:, None]).astype(np.int64)
    out = {"transformers_version": np.frombuffer(transformers.__version__.encode(), dtype=np.uint8), "eos_bias": np.float32(EOS_BIAS),
           "ragged_len": lens, "ragged_mask": mask, "cases_json": np.frombuffer(json.dumps(CASES, sort_keys=True).encode(), dtype=np.uint8)}
    greedy_run = np.load(os.path.join(HERE, "roformer.npz"))["greedy_tokens"]

    def keep(tag, prompt, plen, toks, gap, drawn=None):
        print(f"{tag}: prompt {prompt.shape} lengths {plen.tolist()}, tokens {toks.shape}, margin {gap:.3e}")
        print("   ", toks.tolist())
        assert gap >= MIN_MARGIN, f"{tag}: a selection rests on a score gap of {gap:.3e} < {MIN_MARGIN}"
        out[tag + "_prompt"], out[tag + "_prompt_len"], out[tag + "_tokens"], out[tag + "_margin"] = prompt, plen.astype(np.int32), toks, np.float64(gap)
        if drawn is not None:
            out[tag + "_uniforms"] = drawn.astype(np.float32)

    # continuing the reference's own greedy run from its first 1, 2 or 9 tokens reproduces it
    for n in (1, 2, 9):
        t, _, _, _ = run(m, cfg, phone, tone, spk, greedy_run[:, :n], CASES["greedy"])
        assert np.array_equal(t, greedy_run), n
    try:
        run(m, cfg, phone, tone, spk, random_prompt(cfg, B, 24, 1), CASES["greedy"])
        raise AssertionError("a prompt of max_length tokens must be refused")
    except ValueError:
        pass

    full = np.full(B, P)
    pr = random_prompt(cfg, B, P, 21)
    toks, gap, _, lg = run(m, cfg, phone, tone, spk, pr, CASES["greedy"])
    assert toks.shape == (B, 24) and np.array_equal(toks[:, :P], pr) and lg.shape[0] == 24 - P
    keep("greedy", pr, full, toks, gap)
    out["greedy_logits_row0"] = lg[:, 0].astype(np.float32)

    toks, gap, drawn, _ = run(m, cfg, phone, tone, spk, pr, CASES["sample"])
    assert np.array_equal(toks[:, :P], pr)
    keep("sample", pr, full, toks, gap, np.stack(drawn))

    # n-gram ban: without it the first generated token completes a bigram that lies wholly inside the prompt
    pn = greedy_run[:, :NGRAM_P].copy()
    toks, gap, _, _ = run(m, cfg, phone, tone, spk, pn, CASES["ngram"])
    base, _, _, _ = run(m, cfg, phone, tone, spk, pn, dict(CASES["ngram"], no_repeat_ngram_size=0))
    b = LOOP_ROW
    assert toks[b, NGRAM_P] != base[b, NGRAM_P], "ngram: the ban does not change the first generated token"
    big = (int(pn[b, -1]), int(base[b, NGRAM_P]))
    assert any((int(pn[b, i]), int(pn[b, i + 1])) == big for i in range(NGRAM_P - 1)), ("ngram: the bigram is not inside the prompt", big)
    keep("ngram", pn, np.full(B, NGRAM_P), toks, gap)

    # repetition penalty: without it the first generated token is one that occurs in the prompt (and nowhere else: nothing else exists yet)
    pp = greedy_run[:, :PENALTY_P].copy()
    toks, gap, _, _ = run(m, cfg, phone, tone, spk, pp, CASES["penalty"])
    base, _, _, _ = run(m, cfg, phone, tone, spk, pp, dict(CASES["penalty"], repetition_penalty=1.0))
    assert toks[b, PENALTY_P] != base[b, PENALTY_P] and int(base[b, PENALTY_P]) in set(pp[b].tolist()), "penalty: no effect on the first generated token"
    keep("penalty", pp, np.full(B, PENALTY_P), toks, gap)

    # EOS: one row ends soon after its prompt and is followed by PAD, the other runs to max_length
    toks, gap, _, _ = run(m, cfg, phone, tone, spk, pr, CASES["eos"], eos_bias=EOS_BIAS)
    ends = [int(np.argmax(r == eos)) if (r == eos).any() else None for r in toks]
    assert toks.shape[1] == 40 and any(x is None for x in ends) and any(x is not None and x + 1 < 40 for x in ends), ends
    for r, x in zip(toks, ends):
        if x is not None:
            assert x >= P and (r[x + 1:] == pad).all(), r
    keep("eos", pr, full, toks, gap)

    # ragged: every row alone, with its own phones and prompt
    plen = np.array([P, 4])
    for tag in ("ragged_greedy", "ragged_sample"):
        kw = CASES[tag]
        rows, gaps, us = [], [], []
        for b in range(B):
            Lb, Pb = int(lens[b]), int(plen[b])
            t, g, d, _ = run(m, cfg, phone[b:b + 1, :Lb], tone[b:b + 1, :Lb], spk[b:b + 1, :Lb], pr[b:b + 1, :Pb], kw, seed=RAGGED_SEED)
            rows.append(t[0])
            gaps.append(g)
            us.append(np.concatenate(d) if d else None)
        n = max(len(r) for r in rows)
        toks = np.full((B, n), pad, dtype=np.int64)
        for b, r in enumerate(rows):
            toks[b, :len(r)] = r
        drawn = None
        if kw.get("do_sample"):
            drawn = np.zeros((max(len(u) for u in us), B), dtype=np.float32)
            for b, u in enumerate(us):
                drawn[:len(u), b] = u
        keep(tag, pr, plen, toks, min(gaps), drawn)
    np.savez_compressed(os.path.join(out_dir, "lm_prompt.npz"), **out)
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
        old = np.load(os.path.join(HERE, "lm_prompt.npz"))
        assert set(old.files) == set(new), (sorted(old.files), sorted(new))
        bad = [k for k in new if not (old[k].dtype == np.asarray(new[k]).dtype and np.array_equal(old[k], new[k]))]
        assert not bad, f"regenerated arrays differ: {bad}"
    print("lm_prompt.npz reproduced")


if __name__ == "__main__":
    main()
