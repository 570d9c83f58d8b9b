"""Decode-step time of the text2semantic RoFormer (synthetic weights): 512 sampled tokens, batch 1 and 8.

  --num_beams K        greedy beam search with K beams instead of sampling (1: sampling, or greedy with --greedy)
  --tokens N [N ...]   decode lengths; two of them show whether the cost of a step grows with the position
  --lib PATH           time another build of liblds.so (a previous commit: only the plain decode, which it has)

  --score              time one teacher-forced scoring call (Roformer.score's library call, encoder states given) over the tokens of a
                       decode of the same length, next to that decode: the only other way to visit those positions.  Both as the
                       time between two events on the stream (median of --reps), in the same process; --json FILE keeps the rows.

  --prompt P [P ...]   time a prompted decode (Roformer.generate(semantic_prompt=...)): P prompt tokens (BOS included), then --new tokens,
                       next to the unprompted decode to the same total length, which visits the prompt's P - 1 extra positions step by
                       step: the difference is what the causal prefill saves.  With --batch 8 also one ragged batch whose prompt lengths
                       run from 64 to the largest P.  Greedy; event time on the stream, median of --reps; --json FILE keeps the rows.

  --llama              the decoder-only Llama instead (Llama.generate; the shape of the reference's own example, llama.py:186-193: hidden 768,
                       4 heads, 4 layers, intermediate 512, K 2048) with 64 phones, greedy: the prefill (a decode of one step) and the time per
                       further decode step at --batch, event time on the stream, median of --reps; the RoFormer's step time from the same
                       process for scale; and, where transformers imports, HF's LlamaForCausalLM.generate with the same weights on the
                       same device.  --json FILE keeps the rows.
  --llama --num_beams K  Llama.generate with K beams (early_stopping False, so that the search runs to the full length) next to the greedy decode of
                       the same B items and of B * K rows -- the rows a beam step runs: us per step at --batch.
  --llama --score      one teacher-forced scoring call (lds_llama_score through lds.native, without and with the logits) over the stream of a
                       greedy decode to S = 67 + N ids for every N of --tokens, next to that decode -- the only other way to visit those
                       positions; event time on the stream, median of --reps, same process.  (--lib: the decode alone, for a build without it.)
  --llama --prompt P.. Llama.generate(semantic_prompt=...) with P prompt tokens (BOS included) and --new tokens, next to the unprompted decode to
                       the same total length, which visits the prompt's positions step by step.

With --num_beams > 1, --greedy, --score, --prompt or more than one length the EOS logit is biased far down, so that every sequence runs to the
full length and the time per step is that of a full decode."""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "latent-diffusion-speech_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import infer_tts  # noqa: E402
from lds import native  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, nargs="*", default=[1, 8])
ap.add_argument("--num_beams", type=int, default=1)
ap.add_argument("--greedy", action="store_true")
ap.add_argument("--no_repeat_ngram_size", type=int, default=0)
ap.add_argument("--tokens", type=int, nargs="*", default=[512])
ap.add_argument("--lib", default=None)
ap.add_argument("--score", action="store_true")
ap.add_argument("--prompt", type=int, nargs="*", default=[])
ap.add_argument("--new", type=int, default=64)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--json", default=None)
ap.add_argument("--llama", action="store_true")
a = ap.parse_args()
if a.lib:
    native.LIB_PATH = os.path.abspath(a.lib)
    have = ctypes.CDLL(native.LIB_PATH)
    native.EXPORTS = [n for n in native.EXPORTS if hasattr(have, n)]
    native.TEST_EXPORTS = [n for n in native.TEST_EXPORTS if hasattr(have, n)]

lm = infer_tts.synthetic_lm("cuda")
if a.num_beams > 1 or a.greedy or a.score or a.prompt or len(a.tokens) > 1:
    with torch.no_grad():
        lm.semantic_decoder.cls.predictions.bias[lm.semantic_eos_token_id] -= 1.0e4
mode = f"beam search K {a.num_beams}" if a.num_beams > 1 else "greedy" if a.greedy else "sampled"


def decode(ph, tn, n):
    kw = dict(attention_mask=None, use_cache=None, max_length=n + 1, temperature=1.0, top_k=5, top_p=1.0, repetition_penalty=1.0,
              num_beams=a.num_beams, no_repeat_ngram_size=a.no_repeat_ngram_size, early_stopping=True, spk_id=torch.ones_like(ph), end_gate_threshold=None)
    return lm.generate(ph, tn, do_sample=a.num_beams == 1 and not a.greedy, **kw)


def event_ms(fn, reps):
    """median over reps of the time between two events around fn() on the current stream, and fn's last result"""
    out, ts = None, []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), out


def score_mode():
    rows = []
    for B in a.batch:
        ph = torch.from_numpy((np.arange(B * 64).reshape(B, 64) * 7 % 107 + 1).astype(np.int64)).cuda()
        tn = torch.from_numpy((np.arange(B * 64).reshape(B, 64) * 5 % 12).astype(np.int64)).cuda()
        enc = lm.encode(ph, tn, torch.ones_like(ph))
        for n in a.tokens:
            decode(ph, tn, 64)
            dec_ms, tok = event_ms(lambda: decode(ph, tn, n - 1), a.reps)      # n tokens incl. BOS: n - 1 decode steps = the n - 1 scored positions
            assert tok.shape == (B, n), tok.shape
            lm.native().score(enc, tok)
            sc_ms, _ = event_ms(lambda: lm.native().score(enc, tok), a.reps)
            lg_ms, _ = event_ms(lambda: lm.native().score(enc, tok, return_logits=True), a.reps)
            rows.append({"B": B, "T": n, "positions": B * (n - 1), "decode_ms": dec_ms, "score_ms": sc_ms, "score_with_logits_ms": lg_ms,
                         "decode_over_score": dec_ms / sc_ms, "score_us_per_position": sc_ms * 1e3 / (B * (n - 1))})
            print(rows[-1])
    if a.json:
        import json
        json.dump({"what": "one lds_lm_score call vs the cached decode of the same tokens (greedy, EOS biased down), event time on the stream, "
                           f"median of {a.reps}", "rows": rows}, open(a.json, "w"), indent=1)


def prompt_mode():
    rows = []
    rng = np.random.default_rng(0)

    def prompted(ph, tn, prompt, pmask, total):
        return lm.generate(ph, tn, attention_mask=None, max_length=total, do_sample=False, temperature=1.0, top_k=5, top_p=1.0, repetition_penalty=1.0,
                           spk_id=torch.ones_like(ph), semantic_prompt=prompt, prompt_attention_mask=pmask)

    for B in a.batch:
        ph = torch.from_numpy((np.arange(B * 64).reshape(B, 64) * 7 % 107 + 1).astype(np.int64)).cuda()
        tn = torch.from_numpy((np.arange(B * 64).reshape(B, 64) * 5 % 12).astype(np.int64)).cuda()
        cases = [(P, [P] * B) for P in a.prompt]
        if B > 1 and max(a.prompt) > 64:
            cases.append((max(a.prompt), [int(v) for v in np.linspace(64, max(a.prompt), B).round()]))
        for P, lens in cases:
            sem = rng.integers(0, lm.cfg["semantic_kmeans_num"], size=(B, P)).astype(np.int64)
            sem[:, 0] = lm.semantic_bos_token_id
            prompt = torch.from_numpy(sem).cuda()
            pmask = (torch.arange(P).cuda()[None] < torch.tensor(lens).cuda()[:, None]).to(torch.int64)
            total = P + a.new
            decode(ph, tn, 64)
            prompted(ph, tn, prompt, pmask, total)
            pr_ms, tok = event_ms(lambda: prompted(ph, tn, prompt, pmask, total), a.reps)
            un_ms, tok0 = event_ms(lambda: decode(ph, tn, total - 1), a.reps)
            assert tok.shape == tok0.shape == (B, total), (tok.shape, tok0.shape)
            rows.append({"B": B, "prompt_lengths": sorted(set(lens)), "new_tokens": a.new, "total": total, "prompted_ms": pr_ms, "unprompted_same_total_ms": un_ms,
                         "steps_prompted": total - min(lens), "steps_unprompted": total - 1, "saved_ms": un_ms - pr_ms})
            print(rows[-1])
    if a.json:
        import json
        json.dump({"what": "a prompted greedy decode (causal prefill of the prompt, then the per-row decode steps) vs the unprompted decode to the same total "
                           f"length, EOS biased down, event time on the stream, median of {a.reps}", "rows": rows}, open(a.json, "w"), indent=1)


def llama_mode():
    from text2semantic.llama.llama import Llama
    K, L, new = 2048, 64, a.new
    conf = dict(hidden_size=768, num_attention_heads=4, num_hidden_layers=4, intermediate_size=512, max_position_embeddings=2048)
    m = Llama(dict(conf), semantic_kmeans_num=K, codebook_path="").cuda().eval()
    with torch.no_grad():
        m.llama.lm_head.weight[m.cfg["eos"]] = 0.0      # an EOS logit of exactly 0 never wins here (asserted): every row runs to the full length
    P = L + 3
    hf = None
    try:
        if a.score or a.prompt or a.num_beams > 1:
            raise ImportError      # (those modes compare the library with itself)
        from transformers import LlamaConfig, LlamaForCausalLM
        hf = LlamaForCausalLM(LlamaConfig(vocab_size=m.cfg["vocab"], **conf)).cuda().eval()
        hf.load_state_dict({k[len("llama."):]: v for k, v in m.state_dict().items()}, strict=True)
    except ImportError:
        if not (a.score or a.prompt or a.num_beams > 1):
            print("transformers does not import here: no HF timing")
    rows = []
    if a.score or a.prompt:
        for B in a.batch:
            ph = torch.from_numpy((np.arange(B * L).reshape(B, L) * 7 % 107 + 1).astype(np.int64)).cuda()
            m.generate(ph, ph, max_length=P + 8, do_sample=False)
            for n in (a.tokens if a.score else a.prompt):
                if a.score:      # the stream of a decode of n tokens: S = P + n ids, S - 1 scored positions, n decode steps
                    dec_ms, tok = event_ms(lambda: m.generate(ph, ph, max_length=P + n, do_sample=False), a.reps)
                    assert tok.shape == (B, n), tok.shape
                    row = {"B": B, "S": P + n, "decode_steps": n, "decode_ms": dec_ms, "decode_us_per_step": dec_ms * 1e3 / n}
                    if hasattr(m.native(), "score") and "lds_llama_score" in native.EXPORTS:
                        ids = torch.cat([m.input_ids(ph)[0], tok + m.cfg["shift"]], dim=1)
                        m.native().score(ids)
                        sc_ms, _ = event_ms(lambda: m.native().score(ids), a.reps)
                        lg_ms, _ = event_ms(lambda: m.native().score(ids, return_logits=True), a.reps)
                        row.update(positions=B * (P + n - 1), score_ms=sc_ms, score_with_logits_ms=lg_ms, decode_over_score=dec_ms / sc_ms,
                                   score_us_per_position=sc_ms * 1e3 / (B * (P + n - 1)))
                else:      # n prompt tokens (BOS included), then --new generated ones
                    sem = torch.from_numpy(np.random.default_rng(0).integers(0, K, size=(B, n)).astype(np.int64)).cuda()
                    sem[:, 0] = K
                    total = P - 1 + n + new
                    m.generate(ph, ph, max_length=total, do_sample=False, semantic_prompt=sem)
                    pr_ms, tok = event_ms(lambda: m.generate(ph, ph, max_length=total, do_sample=False, semantic_prompt=sem), a.reps)
                    un_ms, tok0 = event_ms(lambda: m.generate(ph, ph, max_length=total, do_sample=False), a.reps)
                    assert tok.shape == tok0.shape == (B, n - 1 + new), (tok.shape, tok0.shape)
                    row = {"B": B, "prompt_tokens": n, "new_tokens": new, "total": total, "prompted_ms": pr_ms, "unprompted_same_total_ms": un_ms,
                           "steps_prompted": new, "steps_unprompted": n - 1 + new, "saved_ms": un_ms - pr_ms}
                rows.append(row)
                print(row)
        if a.json:
            import json
            what = ("one lds_llama_score call vs the cached greedy decode of the same stream" if a.score else
                    "a prompted greedy Llama decode vs the unprompted decode to the same total length")
            json.dump({"what": what + f" (64 phones, the reference example's width, EOS never wins); event time on the stream, median of {a.reps}", "rows": rows},
                      open(a.json, "w"), indent=1)
        return
    for B in a.batch:
        ph = torch.from_numpy((np.arange(B * L).reshape(B, L) * 7 % 107 + 1).astype(np.int64)).cuda()

        def gen(n):
            return m.generate(ph, ph, max_length=P + n, do_sample=False)
        gen(8)
        pre_ms, _ = event_ms(lambda: gen(1), a.reps)
        all_ms, tok = event_ms(lambda: gen(1 + new), a.reps)
        assert tok.shape == (B, 1 + new), tok.shape
        row = {"B": B, "phones": L, "prompt_ids": P, "new_tokens": new, "prefill_plus_one_step_ms": pre_ms, "decode_ms": all_ms,
               "us_per_step": (all_ms - pre_ms) * 1e3 / new}
        if hf is not None:
            ids, _ = m.input_ids(ph)

            def hf_gen(n):
                return hf.generate(inputs=ids, max_length=P + n, do_sample=False, use_cache=True, pad_token_id=m.cfg["pad"], eos_token_id=m.cfg["eos"],
                                   bad_words_ids=[[i] for i in range(m.cfg["shift"])])
            hf_gen(8)
            h1, _ = event_ms(lambda: hf_gen(1), a.reps)
            h2, htok = event_ms(lambda: hf_gen(1 + new), a.reps)
            row.update(hf_prefill_plus_one_step_ms=h1, hf_decode_ms=h2, hf_us_per_step=(h2 - h1) * 1e3 / new, hf_over_native=h2 / all_ms,
                       same_tokens=bool(htok.shape[1] == P + 1 + new and torch.equal(htok[:, P:] - m.cfg["shift"], tok)))
        if a.num_beams > 1:      # the beam decode of the same B items, and greedy over as many rows as it has beam rows
            Kb = a.num_beams

            def beam(n):
                return m.generate(ph, ph, max_length=P + n, do_sample=False, num_beams=Kb, early_stopping=False)
            beam(8)
            b1, _ = event_ms(lambda: beam(1), a.reps)
            b2, btok = event_ms(lambda: beam(1 + new), a.reps)
            assert btok.shape == (B, 1 + new), btok.shape      # (no hypothesis finished early: every step ran)
            row.update(num_beams=Kb, beam_prefill_plus_one_step_ms=b1, beam_decode_ms=b2, beam_us_per_step=(b2 - b1) * 1e3 / new)
            if B * Kb <= 64:
                phk = ph.repeat(Kb, 1)
                m.generate(phk, phk, max_length=P + 8, do_sample=False)
                g1, _ = event_ms(lambda: m.generate(phk, phk, max_length=P + 1, do_sample=False), a.reps)
                g2, _ = event_ms(lambda: m.generate(phk, phk, max_length=P + 1 + new, do_sample=False), a.reps)
                row.update(greedy_rows=B * Kb, greedy_same_rows_us_per_step=(g2 - g1) * 1e3 / new)
        rows.append(row)
        print(row)
    if a.num_beams > 1:
        if a.json:
            import json
            json.dump({"what": f"Llama.generate with {a.num_beams} beams (early_stopping False, 64 phones, the reference example's width, EOS never wins) next to "
                               f"greedy over B and over B * num_beams rows; event time on the stream, median of {a.reps}", "rows": rows}, open(a.json, "w"), indent=1)
        return
    # the RoFormer's step from the same process, for scale (greedy, EOS biased down)
    with torch.no_grad():
        lm.semantic_decoder.cls.predictions.bias[lm.semantic_eos_token_id] -= 1.0e4
    a.greedy = True
    for B in a.batch:
        ph = torch.from_numpy((np.arange(B * L).reshape(B, L) * 7 % 107 + 1).astype(np.int64)).cuda()
        tn = torch.from_numpy((np.arange(B * L).reshape(B, L) * 5 % 12).astype(np.int64)).cuda()
        decode(ph, tn, 8)
        r1, _ = event_ms(lambda: decode(ph, tn, 1), a.reps)
        r2, _ = event_ms(lambda: decode(ph, tn, 1 + new), a.reps)
        rows.append({"B": B, "model": "roformer", "us_per_step": (r2 - r1) * 1e3 / new})
        print(rows[-1])
    if a.json:
        import json
        json.dump({"what": "Llama.generate (greedy, 64 phones, the reference example's width): a one-step decode (the prefill) and the time per further step; "
                           f"event time on the stream, median of {a.reps}", "rows": rows}, open(a.json, "w"), indent=1)


if a.llama:
    llama_mode()
    sys.exit(0)

if a.prompt:
    a.greedy = True
    prompt_mode()
    sys.exit(0)

if a.score:
    a.greedy = True
    score_mode()
    sys.exit(0)

for B in a.batch:
    ph = torch.from_numpy((np.arange(B * 64).reshape(B, 64) * 7 % 107 + 1).astype(np.int64)).cuda()
    tn = torch.from_numpy((np.arange(B * 64).reshape(B, 64) * 5 % 12).astype(np.int64)).cuda()
    for n in a.tokens:
        decode(ph, tn, 64)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tok = decode(ph, tn, n)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        steps = tok.shape[1] - 1
        print(f"B {B} {mode}: {tuple(tok.shape)} {dt * 1e3:.1f} ms, {dt * 1e6 / steps:.1f} us/step, {B * steps / dt:.0f} tokens/s")
