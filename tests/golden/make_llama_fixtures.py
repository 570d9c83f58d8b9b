"""Golden fixtures of the text2semantic Llama: the reference's own `Llama` class (text2semantic/llama/llama.py, imported from the reference by
path like everything make_fixtures.py drives, never copied) on the installed transformers, with the build-owned seeded weights of
arch.llama_init_state loaded with strict=True, and the reference's own `generate` call with its use_cache argument set to True.

Why not the default use_cache=None: under transformers 5.x generate() then hands LlamaForCausalLM the WHOLE sequence at every step (as for an
uncached decode) while the model still appends every pass's keys / values to one DynamicCache (observed: cache lengths 26, 53, 81, ... for a
26-id prompt), so each step attends to every earlier pass's keys a second time -- an artefact of running the unpinned reference on a newer
library (the sibling of the cache aliasing make_fixtures.roformer_fixtures describes), not the model's semantics.  use_cache=True is what the
None stands for (LlamaConfig.use_cache is True) and evaluates the intended computation; the uncached decode (use_cache=False) gives the same
tokens and logits within 1e-5 (asserted below for the greedy case).

  manifest_llama.json   Llama.state_dict() key -> shape (toy config)
  llama.npz             phone_r0 / phone_r1 (lengths 23 and 15); per case and row (B = 1: all the reference can do, llama.py:148)
                        <case>_r<b>_tokens   what generate returns: the generated ids minus 108, EOS (K + 1) kept
                        <case>_r<b>_logits   HF's raw logits (before any processor) of the K + 3 ids from 108 on, first 16 steps
                        <case>_r<b>_absmax   the abs-max of those logits over the whole run
                        <case>_r<b>_margin   the smallest selection margin of the run: top-1 / top-2 gap (greedy), k | k + 1 gap and the
                                             distance of every uniform from a CDF step (sampling)
                        <case>_r<b>_uniforms the recorded draws (sampling): torch.multinomial replaced by make_fixtures.py's inverse-CDF draw
                        inv_freq             the reference model's rotary inverse frequencies (torch's fp32 pow)
                        eos_row              the "eos" case's edit: the EOS row of lm_head.weight is replaced by this (the head has no bias to steer)
                        weight_seed, sample_seed, cases_json, toy_json, transformers_version

Toy config: hidden 96, 6 heads, 2 kv heads, head_dim 16, inter 160, 2 layers, K 61 (vocab 172), 128 positions.  The weight seed and the sampling
seed are the first ones at which every case's margin is at least 1e-3 (asserted), so the tests can demand exact tokens.

  python tests/golden/make_llama_fixtures.py            # writes tests/golden/llama.npz, manifest_llama.json
  python tests/golden/make_llama_fixtures.py --check    # regenerates into a temporary directory and compares array by array
"""
import argparse
import inspect
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
TOY = dict(hidden_size=96, num_attention_heads=6, num_key_value_heads=2, intermediate_size=160, num_hidden_layers=2, max_position_embeddings=128)
K = 61
LOGIT_STEPS = 16
EOS_SCALES = (3.0, 4.0, 5.0, 6.0, 8.0, 10.0, 12.0)      # the EOS row of the head times one of these: the first that ends both rows early, at different steps
CASES = {
    "greedy": dict(max_length=48, do_sample=False),
    "sample": dict(max_length=48, do_sample=True, top_k=5),
    "eos": dict(max_length=48, do_sample=False),
    "penalty": dict(max_length=48, do_sample=False, repetition_penalty=1.3, no_repeat_ngram_size=2),
}
DEFAULTS = dict(temperature=1.0, top_k=5, top_p=1.0, repetition_penalty=1.0, no_repeat_ngram_size=0, num_beams=1)


def phones():
    return [(np.arange(23) * 7 % 107 + 1).astype(np.int64), (np.arange(15) * 11 % 107 + 1).astype(np.int64)]


def build_model(weight_seed):
    from transformers import LlamaConfig
    from text2semantic.llama import llama as ref_llama
    assert os.path.realpath(inspect.getfile(ref_llama)).startswith(mf.REF + os.sep)
    m = ref_llama.Llama(config=LlamaConfig(**TOY), semantic_kmeans_num=K, codebook_path="/nonexistent").eval()
    cfg = mf.arch.llama_config(semantic_kmeans_num=K, **TOY)
    state = mf.arch.llama_init_state(cfg, weight_seed, mf.init_weights)
    m.load_state_dict({k: mf.tt(v) for k, v in state.items()}, strict=True)
    assert (m.BOS, m.EOS, m.PAD, m.semantic_token_shift) == (cfg["text_bos"], cfg["text_eos"], cfg["text_pad"], cfg["shift"])
    assert (m.config.bos_token_id, m.config.eos_token_id, m.config.pad_token_id, m.config.vocab_size) == (cfg["bos"], cfg["eos"], cfg["pad"], cfg["vocab"])
    return m, cfg


def run(m, cfg, phone, kw, seed=5, use_cache=True):
    """one generate call of the reference under the margin hooks -> (returned tokens [n], margin, uniforms drawn, raw logits [steps, K + 3])"""
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

    logits = []
    hook = m.llama.lm_head.register_forward_hook(lambda _m, _i, o: logits.append(o[0, -1, cfg["shift"]:].detach().float().numpy().copy()))
    torch.manual_seed(seed)
    torch.topk, torch.argmax, torch.multinomial = topk, argmax, inverse_cdf_multinomial
    try:
        ph = mf.tt(phone[None])
        toks = m.generate(ph, torch.ones_like(ph), use_cache=use_cache, **dict(DEFAULTS, **kw)).numpy()[0]
    finally:
        torch.topk, torch.argmax, torch.multinomial = real
        hook.remove()
    lg = np.stack(logits)
    assert lg.shape[0] == len(toks), (lg.shape, len(toks))
    return toks, mg.gap, (np.concatenate(mg.drawn) if mg.drawn else None), lg


def attempt(weight_seed, sample_seed):
    """every case at these seeds -> the fixture dict, or the name of the first case whose margin is too small"""
    m, cfg = build_model(weight_seed)
    eos_s = cfg["eos"] - cfg["shift"]
    out = {"inv_freq": m.llama.model.rotary_emb.inv_freq.detach().float().numpy().copy()}
    head = m.llama.lm_head.weight
    row0 = head.data[cfg["eos"]].clone()
    for tag, kw in CASES.items():
        scales = EOS_SCALES if tag == "eos" else (None,)
        for sc in scales:
            if sc is not None:
                head.data[cfg["eos"]] = row0 * sc
            res = [run(m, cfg, p, kw, sample_seed) for p in phones()]
            head.data[cfg["eos"]] = row0
            if sc is None:
                break
            ends = [len(r[0]) for r in res]
            if all(r[0][-1] == eos_s for r in res) and ends[0] != ends[1] and min(ends) >= 3:
                out["eos_row"] = (row0 * sc).numpy().copy()
                break
        else:
            return "eos (no scale ends both rows early at different steps)"
        for b, (toks, gap, drawn, lg) in enumerate(res):
            print(f"  {tag} r{b}: {len(toks)} tokens, margin {gap:.3e}, logit absmax {np.abs(lg).max():.3f}: {toks.tolist()[:12]}")
            if gap < MIN_MARGIN:
                return f"{tag} r{b} (margin {gap:.3e})"
            if tag != "eos":
                assert len(toks) == kw["max_length"] - (len(phones()[b]) + 3) or toks[-1] == eos_s
            p = f"{tag}_r{b}_"
            out[p + "tokens"], out[p + "logits"] = toks.astype(np.int64), lg[:LOGIT_STEPS].astype(np.float32)
            out[p + "absmax"], out[p + "margin"] = np.float64(np.abs(lg).max()), np.float64(gap)
            if drawn is not None:
                out[p + "uniforms"] = drawn.astype(np.float32)
    # the cached and the uncached decode agree
    for b, p in enumerate(phones()):
        toks, _, _, lg = run(m, cfg, p, CASES["greedy"], sample_seed, use_cache=False)
        assert np.array_equal(toks, out[f"greedy_r{b}_tokens"]) and np.abs(lg[:LOGIT_STEPS] - out[f"greedy_r{b}_logits"]).max() < 1e-5
    # the penalty case exercises its features: its tokens differ from the plain greedy run's
    assert any(not np.array_equal(out[f"penalty_r{b}_tokens"], out[f"greedy_r{b}_tokens"]) for b in range(2)), "penalty: no effect"
    return out


def make(out_dir):
    import transformers
    for weight_seed in range(8):
        for sample_seed in range(5, 9):
            print(f"weight seed {weight_seed}, sample seed {sample_seed}")
            out = attempt(weight_seed, sample_seed)
            if isinstance(out, dict):
                break
            print("  rejected:", out)
            if not out.startswith("sample"):
                break
        if isinstance(out, dict):
            break
    assert isinstance(out, dict), "no seed gives every case a margin of 1e-3"
    m, cfg = build_model(weight_seed)
    json.dump({k: list(v.shape) for k, v in m.state_dict().items()}, open(os.path.join(out_dir, "manifest_llama.json"), "w"), indent=0)
    for b, p in enumerate(phones()):
        out[f"phone_r{b}"] = p
    out.update(weight_seed=np.int64(weight_seed), sample_seed=np.int64(sample_seed),
               cases_json=np.frombuffer(json.dumps(CASES, sort_keys=True).encode(), dtype=np.uint8),
               toy_json=np.frombuffer(json.dumps(dict(TOY, semantic_kmeans_num=K), sort_keys=True).encode(), dtype=np.uint8),
               transformers_version=np.frombuffer(transformers.__version__.encode(), dtype=np.uint8))
    np.savez_compressed(os.path.join(out_dir, "llama.npz"), **out)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="regenerate into a temporary directory and compare with the committed files")
    a = ap.parse_args()
    if not a.check:
        make(HERE)
        return
    with tempfile.TemporaryDirectory() as d:
        new = make(d)
        old = np.load(os.path.join(HERE, "llama.npz"))
        assert set(old.files) == set(new), (sorted(old.files), sorted(new))
        bad = [k for k in new if not (old[k].dtype == np.asarray(new[k]).dtype and np.array_equal(old[k], new[k]))]
        assert not bad, f"regenerated arrays differ: {bad}"
        assert json.load(open(os.path.join(d, "manifest_llama.json"))) == json.load(open(os.path.join(HERE, "manifest_llama.json")))
    print("llama.npz reproduced")


if __name__ == "__main__":
    main()
