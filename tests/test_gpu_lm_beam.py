"""Greedy beam search and no-repeat n-gram blocking of the LM decode on a real MI355X: Roformer.generate against the reference's own
tokens (tests/golden/roformer_beam.npz, tests/golden/make_lm_beam_fixtures.py), one beam step of the kernel against the numpy
restatement (tests/lm_beam_numpy.py), batch rows against the same rows alone, repeatability, and the phones-to-wav script."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import lm_beam_numpy as NB
from conftest import ROOT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KW = dict(use_cache=None, temperature=1.0, top_k=5, top_p=1.0, repetition_penalty=1.0, num_beams=1, no_repeat_ngram_size=0, early_stopping=True,
          end_gate_threshold=None, do_sample=False)
CASES = {      # make_lm_beam_fixtures.CASES
    "beam4": dict(num_beams=4, max_length=24),
    "beam4_ngram3": dict(num_beams=4, max_length=24, no_repeat_ngram_size=3, repetition_penalty=1.2),
    "beam4_eos": dict(num_beams=4, max_length=40),
    "beam3_ragged": dict(num_beams=3, max_length=24),
    "greedy_ngram2": dict(num_beams=1, max_length=24, no_repeat_ngram_size=2),
    "sample_ngram2": dict(num_beams=1, max_length=40, no_repeat_ngram_size=2, do_sample=True),
}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def lm_gpu():
    import yaml
    from text2semantic.utils import get_language_model
    args = yaml.safe_load(open(os.path.join(ROOT, "tests", "golden", "config_lm_like_reference.yaml")))
    return get_language_model(**args).to("cuda").eval()


@pytest.fixture(scope="module")
def fx(golden):
    g, b = golden("roformer.npz"), golden("roformer_beam.npz")
    return dict(b, phone=g["phone"], tone=g["tone"], spk_id=g["spk_id"])


class EosBias:
    """the fixture's EOS bias on the LM head for the duration of a block"""

    def __init__(self, m, bias):
        self.m, self.bias = m, float(bias)

    def _add(self, v):
        with torch.no_grad():
            self.m.semantic_decoder.cls.predictions.bias[self.m.semantic_eos_token_id] += v
        self.m._native = None

    def __enter__(self):
        self._add(self.bias)

    def __exit__(self, *exc):
        self._add(-self.bias)


def generate(m, fx, tag, monkeypatch, rows=None):
    kw = dict(KW, **CASES[tag])
    phone, tone, spk = (dev(fx[k]) for k in ("phone", "tone", "spk_id"))
    mask = dev(fx["ragged_mask"]) if "ragged" in tag else None
    if rows is not None:
        phone, tone, spk = phone[rows].contiguous(), tone[rows].contiguous(), spk[rows].contiguous()
        mask = mask[rows].contiguous() if mask is not None else None
    if kw["do_sample"]:
        u = fx[tag + "_uniforms"]
        full = np.zeros((kw["max_length"] - 1, u.shape[1]), dtype=np.float32)
        full[: u.shape[0]] = u
        if rows is not None:
            full = full[:, rows]
        monkeypatch.setattr(torch, "rand", lambda *a, **k: dev(full))
    with EosBias(m, fx["eos_bias"] if "eos" in tag else 0.0):
        return m.generate(phone, tone, attention_mask=mask, spk_id=spk, **kw).cpu().numpy()


@pytest.mark.parametrize("tag", list(CASES))
def test_generate_vs_reference(lm_gpu, fx, monkeypatch, tag):
    """token-exact against the reference's Roformer.generate (transformers GenerationMixin) on the same weights and inputs"""
    assert float(fx[tag + "_margin"]) >= 1e-3
    toks = generate(lm_gpu, fx, tag, monkeypatch)
    want = fx[tag + "_tokens"]
    assert toks.shape == want.shape, (toks.shape, want.shape)
    assert np.array_equal(toks, want), (toks.tolist(), want.tolist())


def run_kernel_step(logits, K, cur_len, max_length, eos, pen, ngram, es, state, unsat):
    from lds import native
    run_seq, run_score, fin_seq, fin_score, fin_flag, fin_len = state
    R = logits.shape[0]
    pad = int(run_seq[0, -1])
    ins = [dev(a) for a in (logits, run_seq, run_score, fin_seq, fin_score, fin_flag.astype(np.int32), fin_len.astype(np.int32), unsat.astype(np.int32))]
    outs = dict(run_seq=torch.full_like(ins[1], pad), run_score=torch.zeros_like(ins[2]), parent=torch.zeros(R, dtype=torch.int32, device="cuda"),
                fin_seq=torch.full_like(ins[3], pad), fin_score=torch.zeros_like(ins[4]), fin_flag=torch.zeros_like(ins[5]),
                fin_len=torch.zeros_like(ins[6]), unsat=torch.zeros_like(ins[7]), flags=torch.zeros(1, dtype=torch.int32, device="cuda"))
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    native.check(native.lib().lds_test_lm_beam_step(
        p(ins[0]), R // K, K, logits.shape[1], cur_len, max_length, eos, C.c_float(pen), ngram, es, *(p(t) for t in ins[1:]),
        p(outs["run_seq"]), p(outs["run_score"]), p(outs["parent"]), p(outs["fin_seq"]), p(outs["fin_score"]), p(outs["fin_flag"]),
        p(outs["fin_len"]), p(outs["unsat"]), p(outs["flags"]), native._stream()))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in outs.items()}


STEP_CASES = [      # (B, K, V, cur_len, max_length, rep_pen, ngram, early_stopping, finished share, EOS boost)
    (3, 4, 4099, 1, 40, 1.0, 0, 1, 0.0, None),
    (3, 4, 4099, 17, 40, 1.2, 3, 1, 0.3, "top"),
    (2, 8, 4099, 9, 40, 1.0, 2, 0, 0.5, "mid"),
    (4, 2, 300, 12, 13, 1.1, 1, 1, 0.4, None),
    (2, 3, 2304, 30, 64, 1.0, 4, 2, 1.0, "top"),
    (1, 5, 1000, 70, 200, 1.3, 2, 1, 0.3, "mid"),
    (2, 4, 4099, 500, 600, 1.2, 3, 1, 0.3, "mid"),          # long histories: the penalty marks and the n-gram scan over 500 ...
    (1, 8, 4099, 1000, 1100, 1.2, 2, 0, 0.4, "top"),        # ... and 1000 tokens, and the copies of rows that long
]


@pytest.mark.parametrize("case", range(len(STEP_CASES)))
def test_beam_step_kernel_vs_numpy(case):
    B, K, V, cur_len, max_length, pen, ng, es, share, boost = STEP_CASES[case]
    rng = np.random.default_rng(200 + case)
    eos = V - 2
    state = NB.random_state(rng, B, K, V, cur_len, max_length, V - 3, V - 1, share)
    unsat = np.ones(B, np.int32)
    unsat[-1] = 0 if B > 1 and share > 0.9 else 1
    logits = rng.normal(0, 3, size=(B * K, V)).astype(np.float32)
    if boost == "top":
        logits[:, eos] = logits.max(-1) + 2.0
    elif boost == "mid":
        logits[:, eos] = np.sort(logits, -1)[:, -2] - 0.01
    want = NB.beam_step(logits, K, cur_len, max_length, eos, pen, ng, es, *state, unsat)
    got = run_kernel_step(logits, K, cur_len, max_length, eos, pen, ng, es, state, unsat)
    for k in ("run_seq", "parent", "fin_seq", "fin_flag", "fin_len", "unsat"):
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    assert int(got["flags"][0]) == want["flags"]
    for k in ("run_score", "fin_score"):
        np.testing.assert_allclose(got[k], want[k], rtol=1e-5, atol=0)


@pytest.mark.parametrize("tag", ["beam4", "beam4_ngram3", "beam4_eos", "beam3_ragged", "greedy_ngram2", "sample_ngram2"])
def test_batch_rows_equal_rows_alone(lm_gpu, fx, monkeypatch, tag):
    """every batch row is what the row gives alone, bit for bit, up to the batch's common length (PAD after); with padding (the ragged
    case's short row runs alone un-padded)"""
    batch = generate(lm_gpu, fx, tag, monkeypatch)
    for b in range(batch.shape[0]):
        rows = [b]
        alone = None
        if "ragged" in tag:      # un-padded: the row's own phones only
            n = int(fx["ragged_len"][b])
            kw = dict(KW, **CASES[tag])
            with EosBias(lm_gpu, 0.0):
                alone = lm_gpu.generate(dev(fx["phone"][b:b + 1, :n]), dev(fx["tone"][b:b + 1, :n]), attention_mask=None,
                                        spk_id=dev(fx["spk_id"][b:b + 1, :n]), **kw).cpu().numpy()[0]
        else:
            alone = generate(lm_gpu, fx, tag, monkeypatch, rows=rows)[0]
        n = alone.shape[0]
        assert n <= batch.shape[1]
        assert np.array_equal(batch[b, :n], alone), (b, batch[b].tolist(), alone.tolist())
        assert (batch[b, n:] == lm_gpu.semantic_pad_token_id).all()


def test_repeatable(lm_gpu, fx, monkeypatch):
    a = generate(lm_gpu, fx, "beam4_eos", monkeypatch)
    b = generate(lm_gpu, fx, "beam4_eos", monkeypatch)
    c = generate(lm_gpu, fx, "beam4_ngram3", monkeypatch)
    d = generate(lm_gpu, fx, "beam4_ngram3", monkeypatch)
    assert np.array_equal(a, b) and np.array_equal(c, d)


def test_beam_search_at_length_eight_beams(lm_gpu, fx):
    """eight beams over a longer decode (cache ancestry across many steps): each row equals the row alone, and two calls agree"""
    phone, tone, spk = (dev(fx[k]) for k in ("phone", "tone", "spk_id"))
    kw = dict(KW, num_beams=8, max_length=96, no_repeat_ngram_size=2)
    t1 = lm_gpu.generate(phone, tone, spk_id=spk, **kw).cpu().numpy()
    t2 = lm_gpu.generate(phone, tone, spk_id=spk, **kw).cpu().numpy()
    assert np.array_equal(t1, t2)
    one = lm_gpu.generate(phone[1:2].contiguous(), tone[1:2].contiguous(), spk_id=spk[1:2].contiguous(), **kw).cpu().numpy()[0]
    assert np.array_equal(t1[1, :one.shape[0]], one)
    for r in t1:      # the ban holds: no bigram twice before the first EOS / PAD
        body = [int(x) for x in r[: int(np.argmax(r >= lm_gpu.semantic_eos_token_id)) if (r[1:] >= lm_gpu.semantic_eos_token_id).any() else len(r)]]
        pairs = list(zip(body, body[1:]))
        assert len(pairs) == len(set(pairs)), r.tolist()


def test_infer_tts_cli_beam_search(tmp_path):
    """the script with --num_beams 4 --no_repeat_ngram_size 3: phones -> beam-searched tokens -> wav"""
    sys.path.insert(0, ROOT)
    import infer_tts
    ph = np.stack([(np.arange(12) * 7 % 107 + 1), (np.arange(12) * 5 % 12)]).astype(np.int64)
    np.save(tmp_path / "phones.npy", ph)
    wav = infer_tts.main(["--synthetic", "--phones", str(tmp_path / "phones.npy"), "--max_length", "17", "--num_beams", "4", "--no_repeat_ngram_size", "3",
                          "-s", "250", "-o", str(tmp_path / "o.npy")])
    assert wav.ndim == 1 and wav.shape[0] % 512 == 0 and 0 < wav.shape[0] <= 16 * 512 and np.isfinite(wav).all()
