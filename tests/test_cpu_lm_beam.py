"""Beam search and n-gram blocking of the LM decode without a GPU: the numpy restatement (tests/lm_beam_numpy.py) against transformers'
own beam-search helpers and logits processors, the argument checks of Roformer.generate, and the new C ABI symbols with their
device-free argument validation."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import yaml

import lm_beam_numpy as NB
from conftest import GOLDEN, ROOT

BOS, EOS, PAD = 4096, 4097, 4098


def hf_beam_step(logits, K, cur_len, max_length, eos, rep_pen, ngram, early_stopping, run_seq, run_score, fin_seq, fin_score, fin_flag, fin_len,
                 unsat):
    """the same step through transformers' GenerationMixin helpers (generation/utils.py _beam_search, steps b to g)"""
    from transformers.generation.logits_process import LogitsProcessorList, NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor
    from transformers.generation.utils import GenerationMixin as G
    es = {1: True, 0: False, 2: "never"}[early_stopping]
    R, V = logits.shape
    B = R // K
    t = torch.from_numpy
    procs = LogitsProcessorList()
    if rep_pen != 1.0:
        procs.append(RepetitionPenaltyLogitsProcessor(penalty=rep_pen))
    if ngram > 0:
        procs.append(NoRepeatNGramLogitsProcessor(ngram))
    running_sequences = t(run_seq.copy()).view(B, K, max_length)
    # beam indices only serve to measure generated lengths: -1 = none, anything else = a generated position
    running_beam_indices = torch.full((B, K, max_length - 1), -1, dtype=torch.int32)
    running_beam_indices[:, :, :cur_len - 1] = 0
    beam_indices = torch.full((B, K, max_length - 1), -1, dtype=torch.int32)
    for r in range(R):
        beam_indices.view(R, -1)[r, :fin_len[r]] = 0
    log_probs = torch.nn.functional.log_softmax(t(logits.copy()), dim=-1)
    log_probs = procs(t(run_seq[:, :cur_len].copy()), log_probs)
    log_probs = (log_probs.view(B, K, V) + t(run_score.copy()).view(B, K)[:, :, None]).reshape(B, K * V)
    topk_log_probs, topk_running_sequences, topk_running_beam_indices = G._get_top_k_continuations(
        G, log_probs, running_sequences, running_beam_indices, cur_len, 1, False, 2 * K, K, V, B)
    hits = (topk_running_sequences[:, :, cur_len] == eos) | (cur_len + 1 >= max_length)
    rs, rsc, rbi = G._get_running_beams_for_next_iteration(G, topk_log_probs, topk_running_sequences, topk_running_beam_indices, hits, K)
    top_num_beam_mask = torch.cat((torch.ones(K, dtype=torch.bool), torch.zeros(K, dtype=torch.bool)))
    unsat_t = t(unsat.astype(bool).copy()).view(B, 1)
    seqs, bsc, bidx, fin = G._update_finished_beams(
        G, t(fin_seq.copy()).view(B, K, max_length), topk_running_sequences, t(fin_score.copy()).view(B, K), topk_log_probs, beam_indices,
        topk_running_beam_indices, unsat_t, t(fin_flag.astype(bool).copy()).view(B, K), hits, top_num_beam_mask, K, cur_len, 1, 1.0, es)
    new_unsat = G._check_early_stop_heuristic(unsat_t, rsc, bsc, fin, cur_len + 1, max_length, 1, es, 1.0)
    running = bool(G._beam_search_has_unfinished_sequences(new_unsat, fin, hits, es))
    parent = (rbi[:, :, cur_len - 1] % K).reshape(R).numpy()
    return dict(run_seq=rs.reshape(R, -1).numpy(), run_score=rsc.reshape(R).numpy(), fin_seq=seqs.reshape(R, -1).numpy(),
                fin_score=bsc.reshape(R).numpy(), fin_flag=fin.reshape(R).numpy().astype(np.int32),
                fin_len=((bidx + 1) != 0).sum(-1).reshape(R).numpy().astype(np.int32), unsat=new_unsat.reshape(B).numpy().astype(np.int32),
                parent=parent, running=running)


CASES = [      # (B, K, V, cur_len, max_length, rep_pen, ngram, early_stopping, finished share, EOS boost)
    (3, 4, 300, 1, 24, 1.0, 0, 1, 0.0, None),          # first step: beams 1.. carry -1e9
    (3, 4, 300, 9, 24, 1.2, 3, 1, 0.3, None),           # EOS outside the top K
    (2, 4, 300, 9, 24, 1.0, 2, 1, 0.3, "top"),          # EOS inside the top K of every beam
    (2, 3, 280, 7, 24, 1.3, 1, 0, 0.5, "mid"),          # EOS between ranks K and 2K; early_stopping False
    (2, 4, 300, 12, 13, 1.0, 0, 1, 0.4, None),          # the step at max_length: every candidate hits the stopping criteria
    (2, 4, 300, 10, 24, 1.0, 0, 1, 1.0, None),          # an all-finished batch (every slot holds a finished hypothesis)
    (2, 2, 300, 10, 24, 1.0, 2, 2, 0.5, "top"),         # early_stopping "never"
    (1, 8, 400, 6, 24, 1.1, 2, 1, 0.3, "mid"),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_numpy_beam_step_matches_transformers(case):
    pytest.importorskip("transformers")
    B, K, V, cur_len, max_length, pen, ng, es, share, boost = CASES[case]
    rng = np.random.default_rng(100 + case)
    eos = V - 2
    run_seq, run_score, fin_seq, fin_score, fin_flag, fin_len = NB.random_state(rng, B, K, V, cur_len, max_length, V - 3, V - 1, share)
    unsat = np.ones(B, np.int32)
    logits = rng.normal(0, 3, size=(B * K, V)).astype(np.float32)
    if boost == "top":
        logits[:, eos] = logits.max(-1) + 2.0
    elif boost == "mid":
        logits[:, eos] = np.sort(logits, -1)[:, -2] - 0.01
    args = (logits, K, cur_len, max_length, eos, pen, ng, es, run_seq, run_score, fin_seq, fin_score, fin_flag, fin_len, unsat)
    got, want = NB.beam_step(*args), hf_beam_step(*args)
    assert np.array_equal(got["fin_flag"], want["fin_flag"]) and np.array_equal(got["unsat"], want["unsat"])
    # a slot whose score carries a -1e9 mask holds nothing that can reach the output: -1e9 plus a log-probability rounds to a few fp32
    # values around -1e9, and torch.topk orders such ties its own way -- only the slots with real scores must agree
    for pre, extra in (("run", ("parent",)), ("fin", ("fin_len",))):
        real = want[pre + "_score"] > -5e8
        assert np.array_equal(got[pre + "_score"] > -5e8, real)
        for k in (pre + "_seq",) + extra:
            assert np.array_equal(got[k][real], want[k][real]), (k, got[k], want[k])
        np.testing.assert_allclose(got[pre + "_score"][real], want[pre + "_score"][real], rtol=1e-6, atol=0)
    assert NB.running(got["flags"], es) == want["running"]
    if boost == "top" and cur_len + 1 < max_length:      # the case does what it says: EOS candidates finish
        assert (got["fin_len"] == cur_len).any()
    if cur_len + 1 >= max_length:
        assert not want["running"] and not (got["flags"] & 4)


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_ngram_ban_matches_transformers(n):
    pytest.importorskip("transformers")
    from transformers.generation.logits_process import NoRepeatNGramLogitsProcessor
    rng = np.random.default_rng(n)
    V = 12
    for L in range(1, 14):
        ids = rng.integers(0, 5, size=(3, L))      # a small alphabet: many repeated n-grams
        scores = torch.zeros(3, V)
        got = NoRepeatNGramLogitsProcessor(n)(torch.from_numpy(ids), scores.clone())
        for r in range(3):
            assert {int(i) for i in torch.nonzero(torch.isinf(got[r])).flatten()} == NB.ngram_banned(ids[r], n), (n, L, ids[r])


@pytest.fixture(scope="module")
def lm():
    from text2semantic.utils import get_language_model
    return get_language_model(**yaml.safe_load(open(os.path.join(GOLDEN, "config_lm_like_reference.yaml"))))


@pytest.mark.parametrize("tag", ["beam4", "beam4_ngram3", "beam4_eos", "beam3_ragged"])
def test_generate_beam_reproduces_the_reference(lm, golden, tag):
    """the numpy beam-search driver (NB.generate_beam: beam_step, then the caches reordered by parent) over oracle.roformer gives the
    reference's own tokens for every beam case of roformer_beam.npz, and the smallest decision margin the fixture recorded"""
    from oracle import roformer as R
    kw = {"beam4": dict(K=4, max_length=24), "beam4_ngram3": dict(K=4, max_length=24, ngram=3, rep_pen=1.2), "beam4_eos": dict(K=4, max_length=40),
          "beam3_ragged": dict(K=3, max_length=24)}[tag]
    g, fx = golden("roformer.npz"), golden("roformer_beam.npz")
    cfg = lm.cfg
    w = {k: v.detach().cpu().numpy().copy() for k, v in lm.state_dict().items()}
    if "eos" in tag:
        b = w["semantic_decoder.cls.predictions.bias"].copy()
        b[cfg["sem_eos"]] += fx["eos_bias"]
        w["semantic_decoder.cls.predictions.bias"] = w["semantic_decoder.cls.predictions.decoder.bias"] = b
    enc_len = fx["ragged_len"] if "ragged" in tag else None
    enc = R.encoder_forward(w, cfg, g["phone"], g["tone"], g["spk_id"], enc_len)
    toks, gap = NB.generate_beam(w, cfg, enc, enc_len=enc_len, **kw)
    want = fx[tag + "_tokens"]
    assert toks.shape == want.shape and np.array_equal(toks, want), (toks.tolist(), want.tolist())
    assert abs(gap - float(fx[tag + "_margin"])) < 5e-5, (gap, float(fx[tag + "_margin"]))


def test_generate_beam_search_reaches_the_device_check(lm):
    """greedy beam search and n-gram blocking are built: on CPU tensors they get as far as the missing device"""
    ph = torch.ones(1, 4, dtype=torch.long)
    for kw in (dict(num_beams=4, do_sample=False), dict(num_beams=2, do_sample=False, no_repeat_ngram_size=3), dict(no_repeat_ngram_size=2),
               dict(num_beams=8, do_sample=False, early_stopping=False)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            lm.generate(ph, ph, max_length=8, **kw)


def test_generate_refuses_what_is_not_built(lm):
    ph = torch.ones(1, 4, dtype=torch.long)
    with pytest.raises(NotImplementedError, match="beam sampling"):
        lm.generate(ph, ph, num_beams=4, do_sample=True)
    with pytest.raises(NotImplementedError, match="end gate"):
        lm.generate(ph, ph, num_beams=4, do_sample=False, end_gate_threshold=0.5)
    with pytest.raises(NotImplementedError, match="end gate"):
        lm.generate(ph, ph, end_gate_threshold=0.5)
    with pytest.raises(NotImplementedError, match="return_logits"):
        lm.generate(ph, ph, num_beams=2, do_sample=False, return_logits=True)
    for bad in (9, 0, 2.0, True):
        with pytest.raises(ValueError, match="num_beams"):
            lm.generate(ph, ph, num_beams=bad, do_sample=False)
    for bad in (-1, 1.5):
        with pytest.raises(ValueError, match="no_repeat_ngram_size"):
            lm.generate(ph, ph, no_repeat_ngram_size=bad)
    with pytest.raises(ValueError, match="early_stopping"):
        lm.generate(ph, ph, num_beams=2, do_sample=False, early_stopping="soon")


def test_new_symbols_declared_and_exported():
    from lds import native
    hdr = open(os.path.join(ROOT, "include", "lds.h")).read()
    thdr = open(os.path.join(ROOT, "include", "lds_test.h")).read()
    for n in ("lds_lm_generate_opts", "lds_lm_workspace_bytes_opts"):
        assert re.search(r"\bint\s+" + n + r"\(", hdr) and n in native.EXPORTS
    assert "lds_lm_decode_opts;" in hdr
    assert re.search(r"\bint\s+lds_test_lm_beam_step\(", thdr) and "lds_test_lm_beam_step" in native.TEST_EXPORTS
    fields = re.search(r"typedef struct \{([^}]*)\} lds_lm_decode_opts;", hdr).group(1)
    names = re.findall(r"(\w+)\s*[,;]", fields)
    assert names == [f for f, _ in native.LMDecodeOpts._fields_], names


def test_opts_validation_without_a_device():
    """bad options give LDS_EINVAL before anything touches the device: the checks that need no model come first"""
    from lds import native
    L = native.lib()
    nb = C.c_size_t()
    for k in (0, 9):
        assert L.lds_lm_workspace_bytes_opts(None, 2, 23, 40, k, C.byref(nb)) == -1 and "num_beams" in L.lds_last_error().decode()
    dummy = (C.c_float * 8)()
    toks, n = (C.c_int64 * 8)(), C.c_int()
    wsb = (C.c_char * 64)()

    def gen(logits=None, **kw):
        o = native.LMDecodeOpts(0, 5, 1.0, 1.0, 1.0, 0, 1, 1)
        for k, v in kw.items():
            setattr(o, k, v)
        return L.lds_lm_generate_opts(None, dummy, None, 2, 23, 40, C.byref(o), None, toks, logits, C.byref(n), wsb, C.c_size_t(64), None)
    for kw, msg in ((dict(num_beams=9), "num_beams"), (dict(num_beams=0), "num_beams"), (dict(no_repeat_ngram_size=-1), "no_repeat_ngram_size"),
                    (dict(num_beams=4, do_sample=1), "beam sampling"), (dict(num_beams=4, early_stopping=3), "early_stopping"),
                    (dict(num_beams=4, logits=dummy), "logits_out")):
        assert gen(**kw) == -1 and msg in L.lds_last_error().decode(), (kw, L.lds_last_error())
    assert gen() == -1 and "bad argument" in L.lds_last_error().decode()      # valid options: the missing model is what is refused
