"""The Llama's greedy beam search without a GPU: the numpy step (tests/llama_beam_numpy.py) against transformers' own beam-search helpers at
several decoder prompt lengths, the restatement against every case the reference's Llama.generate recorded (tests/golden/llama_beam.npz,
tests/golden/make_llama_beam_fixtures.py), the refusals of Llama.generate, and the C ABI entries with their device-free argument checks."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import llama_beam_numpy as LB
import llama_numpy as LN
from conftest import GOLDEN, ROOT

MIN_MARGIN = 1e-3
ES = {True: 1, False: 0, "never": 2}


def hf_item_step(logits, K, pl, step, max_length, eos, rep_pen, ngram, early_stopping, first_free, run_seq, run_score, fin_seq, fin_score, fin_flag,
                 fin_len, unsat):
    """one item's step through transformers' GenerationMixin helpers (generation/utils.py _beam_search, steps b to g) with
    decoder_prompt_len = pl and the processors in the order generate builds them: repetition penalty, n-gram ban, bad words"""
    from transformers.generation.logits_process import (LogitsProcessorList, NoBadWordsLogitsProcessor, NoRepeatNGramLogitsProcessor,
                                                        RepetitionPenaltyLogitsProcessor)
    from transformers.generation.utils import GenerationMixin as G
    es = {1: True, 0: False, 2: "never"}[early_stopping]
    V = logits.shape[1]
    cur_len = pl + step
    t = torch.from_numpy
    procs = LogitsProcessorList()
    if rep_pen != 1.0:
        procs.append(RepetitionPenaltyLogitsProcessor(penalty=rep_pen))
    if ngram > 0:
        procs.append(NoRepeatNGramLogitsProcessor(ngram))
    if first_free > 0:
        procs.append(NoBadWordsLogitsProcessor([[i] for i in range(first_free)], eos_token_id=eos))
    running_sequences = t(run_seq.copy()).view(1, K, max_length)
    # beam indices only serve to measure generated lengths: -1 = none, anything else = a generated position
    running_beam_indices = torch.full((1, K, max_length - pl), -1, dtype=torch.int32)
    running_beam_indices[:, :, :step] = 0
    beam_indices = torch.full((1, K, max_length - pl), -1, dtype=torch.int32)
    for k in range(K):
        beam_indices[0, k, :fin_len[k]] = 0
    log_probs = torch.nn.functional.log_softmax(t(logits.copy()), dim=-1)
    log_probs = procs(t(run_seq[:, :cur_len].copy()), log_probs)
    log_probs = (log_probs.view(1, K, V) + t(run_score.copy()).view(1, K)[:, :, None]).reshape(1, K * V)
    topv, topseq, topbi = G._get_top_k_continuations(G, log_probs, running_sequences, running_beam_indices, cur_len, pl, False, 2 * K, K, V, 1)
    hits = (topseq[:, :, cur_len] == eos) | (cur_len + 1 >= max_length)
    rs, rsc, rbi = G._get_running_beams_for_next_iteration(G, topv, topseq, topbi, hits, K)
    mask = torch.cat((torch.ones(K, dtype=torch.bool), torch.zeros(K, dtype=torch.bool)))
    unsat_t = torch.tensor([[bool(unsat)]])
    seqs, bsc, bidx, fin = G._update_finished_beams(G, t(fin_seq.copy()).view(1, K, max_length), topseq, t(fin_score.copy()).view(1, K), topv, beam_indices,
                                                    topbi, unsat_t, t(fin_flag.astype(bool).copy()).view(1, K), hits, mask, K, cur_len, pl, 1.0, es)
    new_unsat = G._check_early_stop_heuristic(unsat_t, rsc, bsc, fin, cur_len + 1, max_length, pl, es, 1.0)
    running = bool(G._beam_search_has_unfinished_sequences(new_unsat, fin, hits, es))
    return dict(run_seq=rs.reshape(K, -1).numpy(), run_score=rsc.reshape(K).numpy(), fin_seq=seqs.reshape(K, -1).numpy(), fin_score=bsc.reshape(K).numpy(),
                fin_flag=fin.reshape(K).numpy().astype(np.int32), fin_len=((bidx + 1) != 0).sum(-1).reshape(K).numpy().astype(np.int32),
                unsat=int(new_unsat), parent=(rbi[0, :, step] % K).numpy(), running=running, all_hit=bool(hits.all()))


PLENS = (1, 18, 26)
STEP_CASES = [      # (K, V, step, max_length, rep_pen, ngram, early_stopping, finished share, EOS boost, first_free)
    (4, 172, 0, 48, 1.0, 0, 1, 0.0, None, 108),         # first step: beams 1.. carry -1e9
    (4, 172, 9, 48, 1.2, 3, 1, 0.3, None, 108),          # EOS outside the top K
    (4, 172, 9, 48, 1.0, 2, 1, 0.3, "top", 108),         # EOS inside the top K of every beam
    (3, 200, 7, 48, 1.3, 1, 0, 0.5, "mid", 108),         # EOS between ranks K and 2K; early_stopping False
    (4, 172, 12, 39, 1.0, 0, 1, 0.4, None, 108),         # the step at max_length for the longest prompt (26 + 12 + 1): its candidates all hit
    (4, 172, 10, 48, 1.0, 0, 1, 1.0, None, 108),         # every slot holds a finished hypothesis
    (2, 172, 10, 48, 1.0, 2, 2, 0.5, "top", 108),        # early_stopping "never"
    (8, 300, 6, 48, 1.1, 2, 1, 0.3, "mid", 108),
    (3, 172, 5, 48, 1.0, 0, 0, 0.3, "banned", 108),      # the largest logits sit in the banned range
    (3, 172, 5, 48, 1.2, 2, 1, 0.3, None, 0),            # no banned range
]


@pytest.mark.parametrize("case", range(len(STEP_CASES)))
def test_numpy_step_matches_transformers(case):
    pytest.importorskip("transformers")
    K, V, step, max_length, pen, ng, es, share, boost, ff = STEP_CASES[case]
    B = len(PLENS)
    rng = np.random.default_rng(300 + case)
    eos = V - 2
    state = LB.random_state(rng, B, K, V, step, max_length, ff, V - 1, PLENS, share)
    unsat = np.ones(B, np.int32)
    logits = rng.normal(0, 3, size=(B * K, V)).astype(np.float32)
    if boost == "top":
        logits[:, eos] = logits.max(-1) + 2.0
    elif boost == "mid":
        logits[:, eos] = np.sort(logits[:, ff:], -1)[:, -2] - 0.01
    elif boost == "banned":
        logits[:, :ff] += 8.0
    got = LB.beam_step(logits, K, step, max_length, eos, pen, ng, es, ff, PLENS, np.zeros(B, np.int32), *state, unsat)
    bits = 0
    for b, pl in enumerate(PLENS):
        rows = slice(b * K, (b + 1) * K)
        want = hf_item_step(logits[rows], K, pl, step, max_length, eos, pen, ng, es, ff, *(a[rows] for a in state), unsat[b])
        assert np.array_equal(got["fin_flag"][rows], want["fin_flag"]) and got["unsat"][b] == want["unsat"]
        # slots whose score carries a -1e9 mask hold nothing that can reach the output (tests/test_cpu_lm_beam.py): only real scores must agree
        for pre, extra in (("run", ("parent",)), ("fin", ("fin_len",))):
            real = want[pre + "_score"] > -5e8
            assert np.array_equal(got[pre + "_score"][rows] > -5e8, real)
            for k in (pre + "_seq",) + extra:
                assert np.array_equal(got[k][rows][real], want[k][real]), (k, b, got[k][rows], want[k])
            np.testing.assert_allclose(got[pre + "_score"][rows][real], want[pre + "_score"][real], rtol=1e-6, atol=0)
        assert bool(got["ended"][b]) == (not want["running"]), (b, want)
        assert (got["run_seq"][rows, pl + step] >= ff).all()      # no banned id is ever chosen
        bits |= (1 if want["unsat"] else 0) | (0 if want["fin_flag"].all() else 2) | (0 if want["all_hit"] else 4) | (16 if want["running"] else 0)
        if pl + step + 1 >= max_length:
            assert not want["running"] and got["ended"][b]
        if boost == "top":      # the case does what it says: EOS candidates finish, with the generated length
            assert (got["fin_len"][rows] == step + 1).any()
    assert got["flags"] == bits


def test_numpy_step_freezes_an_ended_item():
    K, V, step, max_length = 3, 172, 6, 48
    rng = np.random.default_rng(7)
    state = LB.random_state(rng, 2, K, V, step, max_length, 108, V - 1, (18, 26), 0.5)
    unsat = np.array([1, 0], np.int32)
    logits = rng.normal(0, 3, size=(2 * K, V)).astype(np.float32)
    both = LB.beam_step(logits, K, step, max_length, V - 2, 1.0, 0, 1, 108, (18, 26), np.array([0, 1]), *state, unsat)
    alone = LB.beam_step(logits[:K], K, step, max_length, V - 2, 1.0, 0, 1, 108, (18,), np.array([0]), *(a[:K] for a in state), unsat[:1])
    for k, a in zip(("run_seq", "run_score", "fin_seq", "fin_score", "fin_flag", "fin_len"), state):
        assert np.array_equal(both[k][K:], a[K:]) and np.array_equal(both[k][:K], alone[k])
    assert both["ended"][1] == 2 and both["unsat"][1] == 0 and both["flags"] == alone["flags"]


# ---- the restatement against the reference's recorded cases ----
@pytest.fixture(scope="module")
def fx():
    f = dict(np.load(os.path.join(GOLDEN, "llama_beam.npz")))
    f["cases"] = json.loads(bytes(f["cases_json"]).decode())
    f["toy"] = json.loads(bytes(f["toy_json"]).decode())
    return f


def case_model(fx, tag):
    """(cfg, state) of a case's model: its own weight seed, and the "eos" case's head row"""
    from lds import arch
    toy = dict(fx["toy"])
    cfg = arch.llama_config(semantic_kmeans_num=toy.pop("semantic_kmeans_num"), **toy)
    state = arch.llama_init_state(cfg, int(fx[tag + "_weight_seed"]))
    if tag == "eos":
        state = dict(state)
        state["llama.lm_head.weight"] = state["llama.lm_head.weight"].copy()
        state["llama.lm_head.weight"][cfg["eos"]] = fx["eos_row"]
    return cfg, state


def case_ids(fx, cfg, tag, b):
    ids = LN.prompt_ids(cfg, fx[f"phone_r{b}"])
    if tag == "prompt":
        ids += [int(t) + cfg["shift"] for t in fx[f"prompt_r{b}"][1:]]
    return ids


CASE_TAGS = ["beam3", "beam4_open", "beam2_never", "beam4_penalty", "eos", "prompt"]


@pytest.mark.parametrize("tag", CASE_TAGS)
def test_restatement_reproduces_the_reference(fx, tag):
    kw = fx["cases"][tag]
    cfg, state = case_model(fx, tag)
    for b in range(2):
        assert float(fx[f"{tag}_r{b}_margin"]) >= MIN_MARGIN
        ids = case_ids(fx, cfg, tag, b)
        toks, gap, steps = LB.generate_beam(state, cfg, fx["inv_freq"], ids, kw["num_beams"], fx["cases"]["max_length"], kw.get("repetition_penalty", 1.0),
                                            kw.get("no_repeat_ngram_size", 0), ES[kw["early_stopping"]])
        want = fx[f"{tag}_r{b}_tokens"] + cfg["shift"]
        assert np.array_equal(toks[:len(ids)], ids)
        assert np.array_equal(toks[len(ids):], want), (b, toks[len(ids):].tolist(), want.tolist())
        assert steps == int(fx[f"{tag}_r{b}_steps"])
        assert abs(gap - float(fx[f"{tag}_r{b}_margin"])) < 5e-5, (gap, float(fx[f"{tag}_r{b}_margin"]))
    if tag == "eos":      # the case does what it says: the best hypothesis is shorter than the longest running beam
        assert len(want) < steps


def test_fixture_cases_are_the_issue_s(fx):
    c = fx["cases"]
    assert c["max_length"] == 48 and (c["beam3"]["num_beams"], c["beam3"]["early_stopping"]) == (3, True)
    assert (c["beam4_open"]["num_beams"], c["beam4_open"]["early_stopping"]) == (4, False)
    assert (c["beam2_never"]["num_beams"], c["beam2_never"]["early_stopping"]) == (2, "never")
    assert (c["beam4_penalty"]["num_beams"], c["beam4_penalty"]["repetition_penalty"], c["beam4_penalty"]["no_repeat_ngram_size"]) == (4, 1.3, 2)
    assert len(fx["prompt_r0"]) == 10 and fx["prompt_r0"][0] == fx["toy"]["semantic_kmeans_num"]


# ---- Llama.generate's refusals ----
@pytest.fixture(scope="module")
def model(fx):
    from text2semantic.llama.llama import Llama
    toy = dict(fx["toy"])
    K = toy.pop("semantic_kmeans_num")
    return Llama(dict(toy), semantic_kmeans_num=K, codebook_path="/nonexistent")


def test_generate_refuses_what_is_not_built(model):
    K = model.cfg["semantic_kmeans_num"]
    ph = torch.tensor([[1, 2, 3]])
    with pytest.raises(NotImplementedError, match="beam sampling"):
        model.generate(ph, ph, num_beams=2, max_length=16)      # do_sample defaults to True
    with pytest.raises(NotImplementedError, match="beam sampling"):
        model.generate(ph, ph, num_beams=4, do_sample=True, max_length=16, semantic_prompt=torch.tensor([[K, 1]]))
    with pytest.raises(NotImplementedError, match="return_logits"):
        model.generate(ph, ph, num_beams=2, do_sample=False, return_logits=True, max_length=16)
    with pytest.raises(NotImplementedError, match="end gate"):
        model.generate(ph, ph, num_beams=2, do_sample=False, end_gate_threshold=0.5)
    for bad in (9, 0, 2.0, True):
        with pytest.raises(ValueError, match="num_beams"):
            model.generate(ph, ph, num_beams=bad, do_sample=False, max_length=16)
    with pytest.raises(ValueError, match="early_stopping"):
        model.generate(ph, ph, num_beams=2, do_sample=False, early_stopping="soon", max_length=16)
    with pytest.raises(ValueError, match="max_length"):
        model.generate(ph, ph, num_beams=2, do_sample=False, max_length=6)      # the prompt has 6 ids
    with pytest.raises(ValueError, match="max_position_embeddings"):
        model.generate(ph, ph, num_beams=2, do_sample=False, max_length=129)
    with pytest.raises(ValueError, match="beam rows"):
        model.generate(ph.repeat(33, 1), ph.repeat(33, 1), num_beams=8, do_sample=False, max_length=16)
    with pytest.raises(ValueError, match="semantic BOS"):
        model.generate(ph, ph, num_beams=2, do_sample=False, max_length=16, semantic_prompt=torch.tensor([[1, 2]]))


def test_generate_reaches_the_device_check(model):
    """beam search is built, also from a semantic prompt and for ragged batches: on CPU tensors it gets as far as the missing device"""
    K = model.cfg["semantic_kmeans_num"]
    ph = torch.tensor([[1, 2, 3], [4, 5, 6]])
    mask = torch.tensor([[1, 1, 1], [1, 1, 0]])
    for kw in (dict(num_beams=2), dict(num_beams=8, early_stopping=False), dict(num_beams=3, early_stopping="never", no_repeat_ngram_size=2),
               dict(num_beams=4, semantic_prompt=torch.tensor([[K, 1, 2], [K, 3, 0]]), prompt_attention_mask=torch.tensor([[1, 1, 1], [1, 1, 0]]))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            model.generate(ph, ph, attention_mask=mask, do_sample=False, max_length=16, **kw)


# ---- the C ABI ----
def test_new_symbols_declared_and_exported():
    from lds import native
    hdr = open(os.path.join(ROOT, "include", "lds.h")).read()
    thdr = open(os.path.join(ROOT, "include", "lds_test.h")).read()
    for n in ("lds_llama_generate_beam", "lds_llama_beam_workspace_bytes"):
        assert re.search(r"\bint\s+" + n + r"\(", hdr) and n in native.EXPORTS and hasattr(native.lib(), n)
    for n in ("lds_test_llama_beam_step", "lds_test_llama_beam_attn", "lds_test_llama_generate_beam_poll"):
        assert re.search(r"\bint\s+" + n + r"\(", thdr) and n in native.TEST_EXPORTS and hasattr(native.lib(), n)
    assert hasattr(native.Llama, "generate_beam")


def test_option_checks_come_first_without_a_device():
    """bad options and shapes give LDS_EINVAL with a NULL handle: the checks that need no model come before everything else"""
    from lds import native
    L = native.lib()
    nb = C.c_size_t()
    err = lambda: L.lds_last_error().decode()      # noqa: E731
    for k in (1, 9, 0):
        assert L.lds_llama_beam_workspace_bytes(None, 2, 26, 48, k, C.byref(nb)) == -1 and "num_beams" in err()
    assert L.lds_llama_beam_workspace_bytes(None, 64, 26, 48, 8, C.byref(nb)) == -1 and "beam rows" in err()
    assert L.lds_llama_beam_workspace_bytes(None, 2, 26, 7501, 4, C.byref(nb)) == -1 and "max_length" in err()
    assert L.lds_llama_beam_workspace_bytes(None, 2, 26, 48, 4, C.byref(nb)) == -1 and "bad argument" in err()
    ids, toks, n = (C.c_int64 * 64)(), (C.c_int64 * 128)(), C.c_int()
    wsb = (C.c_char * 64)()

    def gen(B=2, P=26, max_length=48, in_len=None, **kw):
        o = native.LMDecodeOpts(0, 5, 1.0, 1.0, 1.0, 0, 4, 1)
        for k, v in kw.items():
            setattr(o, k, v)
        lens = None if in_len is None else (C.c_int32 * B)(*in_len)
        return L.lds_llama_generate_beam(None, ids, lens, B, P, max_length, C.byref(o), toks, C.byref(n), wsb, C.c_size_t(64), None)
    for kw, msg in ((dict(num_beams=1), "num_beams"), (dict(num_beams=9), "num_beams"), (dict(do_sample=1), "beam sampling"),
                    (dict(early_stopping=3), "early_stopping"), (dict(no_repeat_ngram_size=-1), "no_repeat_ngram_size"), (dict(B=33, num_beams=8), "beam rows"),
                    (dict(max_length=7501), "max_length"), (dict(in_len=[26, 27]), "in_len"), (dict(in_len=[26, 0]), "in_len"), (dict(max_length=26), "in_len")):
        assert gen(**kw) == -1 and msg in err(), (kw, err())
    assert gen() == -1 and "bad argument" in err()      # valid options: the missing model is what is refused
    # the plain entry still refuses beams, and points at the new one
    o = native.LMDecodeOpts(0, 5, 1.0, 1.0, 1.0, 0, 2, 1)
    assert L.lds_llama_generate(None, ids, None, 2, 26, 48, C.byref(o), None, toks, None, C.byref(n), wsb, C.c_size_t(64), None) == -1
    assert "beam" in err() and "lds_llama_generate_beam" in err()
