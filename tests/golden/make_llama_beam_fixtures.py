"""Golden fixtures of the Llama's greedy beam search: the reference's own `Llama.generate` (text2semantic/llama/llama.py:121-184, imported from the
reference by path, never copied) with num_beams > 1 on the installed transformers, built the way make_llama_fixtures.py builds its cases: the toy
config and seeded weights of make_llama_fixtures.build_model, use_cache=True (see there), the margin hooks of make_lm_beam_fixtures on torch.topk.

  llama_beam.npz   phone_r0 / phone_r1 (make_llama_fixtures.phones); per case and row (B = 1: all the reference can do)
                   <case>_r<b>_tokens   what generate returns: the ids behind the prompt minus 108, EOS (K + 1) kept
                   <case>_r<b>_margin   the smallest score gap at a selection that reaches them (make_lm_beam_fixtures.Margins)
                   <case>_r<b>_steps    decode steps HF ran (forward passes of the head)
                   eos_row              the "eos" case's edit: the EOS row of lm_head.weight is replaced by this
                   prompt_r<b>          the "prompt" case's semantic prompt in the returned numbering, the semantic BOS (K) first
                   <case>_weight_seed   the seed of the case's weights (arch.llama_init_state)
                   inv_freq, cases_json, toy_json, transformers_version

Cases (max_length 48): three beams with early_stopping=True; four with False; two with "never"; four with repetition_penalty 1.3 and
no_repeat_ngram_size 2; "eos": four beams, early_stopping=False, with the EOS row of the head scaled until hypotheses finish at different lengths
and the returned one is shorter than the longest running beam; "prompt": three beams continuing [prompt ids + 9 semantic ids] -- the reference
wrapper cannot pass a prompt, so m.llama.generate is driven with llama.py:157-171's GenerationConfig.  Every case differs from the greedy run
(asserted).  Every case takes the first weight seed at which both rows' margins are at least 1e-3, so the tests can demand exact tokens.

  python tests/golden/make_llama_beam_fixtures.py            # writes tests/golden/llama_beam.npz
  python tests/golden/make_llama_beam_fixtures.py --check    # regenerates into a temporary directory and compares array by array
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
import make_llama_fixtures as ml  # noqa: E402

np, torch = mf.np, mf.torch
MIN_MARGIN = mb.MIN_MARGIN
MAX_LENGTH = 48
PROMPT_TOKENS = 9
CASES = {
    "beam3": dict(num_beams=3, early_stopping=True),
    "beam4_open": dict(num_beams=4, early_stopping=False),
    "beam2_never": dict(num_beams=2, early_stopping="never"),
    "beam4_penalty": dict(num_beams=4, early_stopping=True, repetition_penalty=1.3, no_repeat_ngram_size=2),
    "eos": dict(num_beams=4, early_stopping=False),
    "prompt": dict(num_beams=3, early_stopping=True),
}
DEFAULTS = dict(max_length=MAX_LENGTH, do_sample=False, temperature=1.0, top_k=5, top_p=1.0, repetition_penalty=1.0, no_repeat_ngram_size=0)


def run(m, cfg, phone, kw, prompt=None):
    """one beam search of the reference under the margin hooks -> (returned tokens [n] minus the shift, margin, steps, lengths of the finished
    hypotheses at the end).  prompt: model ids appended to [108, phones, 109, 108 + K]; then m.llama.generate is called as llama.py:157-180 does."""
    from transformers import GenerationConfig
    from transformers.generation.utils import GenerationMixin
    kw = dict(DEFAULTS, **kw)
    mg = mb.Margins(kw["num_beams"])
    real_topk, real_upd = torch.topk, GenerationMixin._update_finished_beams
    steps, last = [0], {}

    def topk(x, k, *a, **k2):
        mg.note(x, k)
        return real_topk(x, k, *a, **k2)

    def upd(self, *a, **k2):
        out = real_upd(self, *a, **k2)
        last["len"] = [int(n) for n, f in zip((out[2][0] >= 0).sum(-1).tolist(), out[3][0].tolist()) if f]
        return out

    hook = m.llama.lm_head.register_forward_hook(lambda *_a: steps.__setitem__(0, steps[0] + 1))
    torch.topk, GenerationMixin._update_finished_beams = topk, upd
    try:
        ph = mf.tt(phone[None])
        if prompt is None:
            toks = m.generate(ph, torch.ones_like(ph), use_cache=True, **kw).numpy()[0]
        else:
            ids = torch.cat([torch.tensor([[m.BOS]]), ph, torch.tensor([[m.EOS, m.config.bos_token_id]]), mf.tt(np.asarray(prompt)[None])], dim=1)
            gc = GenerationConfig(bos_token_id=m.config.bos_token_id, eos_token_id=m.config.eos_token_id, pad_token_id=m.config.pad_token_id,
                                  bad_words_ids=[[i] for i in range(0, m.semantic_token_shift)], **kw)
            out = m.llama.generate(inputs=ids, attention_mask=None, use_cache=True, generation_config=gc, logits_processor=None)
            toks = (out[:, ids.shape[1]:] - m.semantic_token_shift).numpy()[0]
    finally:
        torch.topk, GenerationMixin._update_finished_beams = real_topk, real_upd
        hook.remove()
    return toks, mg.gap, steps[0], last.get("len", [])


def greedy(m, cfg, phone, prompt=None):
    if prompt is None:
        return ml.run(m, cfg, phone, dict(max_length=MAX_LENGTH, do_sample=False))[0]
    return run(m, cfg, phone, dict(num_beams=1, early_stopping=False), prompt)[0]


def attempt(tag, weight_seed):
    """one case (both rows) at this weight seed -> its fixture entries, or why the seed does not qualify"""
    kw = CASES[tag]
    m, cfg = ml.build_model(weight_seed)
    shift, eos_s = cfg["shift"], cfg["eos"] - cfg["shift"]
    out = {}
    head = m.llama.lm_head.weight
    row0 = head.data[cfg["eos"]].clone()
    prompts = [None, None]
    if tag == "prompt":      # the first greedy tokens of each row, as a semantic prompt
        plain = [greedy(m, cfg, p) for p in ml.phones()]
        if any(eos_s in g[:PROMPT_TOKENS] for g in plain):
            return "the greedy run ends inside the prompt"
        prompts = [(g[:PROMPT_TOKENS] + shift).astype(np.int64) for g in plain]
    for sc in (ml.EOS_SCALES if tag == "eos" else (None,)):
        if sc is not None:
            head.data[cfg["eos"]] = row0 * sc
        res = [run(m, cfg, p, kw, pr) for p, pr in zip(ml.phones(), prompts)]
        base = [greedy(m, cfg, p, pr) for p, pr in zip(ml.phones(), prompts)]
        head.data[cfg["eos"]] = row0
        if sc is None:
            break
        # hypotheses finish at different lengths, and the returned one is shorter than the longest running beam
        if all(r[0][-1] == eos_s and len(set(r[3])) >= 2 and len(r[0]) < r[2] for r in res):
            out["eos_row"] = (row0 * sc).numpy().copy()
            break
    else:
        return "no scale gives hypotheses of different lengths with the best one shorter than the longest beam"
    for b, (toks, gap, steps, lens) in enumerate(res):
        print(f"  {tag} r{b}: {len(toks)} tokens in {steps} steps, finished lengths {lens}, margin {gap:.3e}: {toks.tolist()[:12]}")
        if gap < MIN_MARGIN:
            return f"r{b}: margin {gap:.3e}"
        if len(toks) == len(base[b]) and np.array_equal(toks, base[b]):
            return f"r{b}: equals the greedy run"
        p = f"{tag}_r{b}_"
        out[p + "tokens"], out[p + "margin"], out[p + "steps"] = toks.astype(np.int64), np.float64(gap), np.int64(steps)
        if prompts[b] is not None:
            out[f"prompt_r{b}"] = np.concatenate([[cfg["bos"] - shift], prompts[b] - shift]).astype(np.int64)
    out[tag + "_weight_seed"] = np.int64(weight_seed)
    return out


def make(out_dir):
    import transformers
    out = {}
    for tag in CASES:      # every case walks the weight seeds on its own: twelve runs seldom all clear 1e-3 at one seed
        for weight_seed in range(400):
            print(f"{tag}: weight seed {weight_seed}")
            got = attempt(tag, weight_seed)
            if isinstance(got, dict):
                break
            print("  rejected:", got)
        assert isinstance(got, dict), f"{tag}: no seed gives both rows a margin of {MIN_MARGIN}"
        out.update(got)
    m, _ = ml.build_model(0)
    out["inv_freq"] = m.llama.model.rotary_emb.inv_freq.detach().float().numpy().copy()
    for b, p in enumerate(ml.phones()):
        out[f"phone_r{b}"] = p
    out.update(cases_json=np.frombuffer(json.dumps(dict(CASES, max_length=MAX_LENGTH), sort_keys=True).encode(), dtype=np.uint8),
               toy_json=np.frombuffer(json.dumps(dict(ml.TOY, semantic_kmeans_num=ml.K), sort_keys=True).encode(), dtype=np.uint8),
               transformers_version=np.frombuffer(transformers.__version__.encode(), dtype=np.uint8))
    np.savez_compressed(os.path.join(out_dir, "llama_beam.npz"), **out)
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
        old = np.load(os.path.join(HERE, "llama_beam.npz"))
        assert set(old.files) == set(new), (sorted(old.files), sorted(new))
        bad = [k for k in new if not (old[k].dtype == np.asarray(new[k]).dtype and np.array_equal(old[k], new[k]))]
        assert not bad, f"regenerated arrays differ: {bad}"
    print("llama_beam.npz reproduced")


if __name__ == "__main__":
    main()
