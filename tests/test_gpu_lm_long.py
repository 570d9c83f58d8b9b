"""The LM at the reference's sizes on a real MI355X, against the numpy oracle computed at test time (no fixtures): 22_infer_tts.py calls
Roformer.generate with max_length 1024 and real sentences run to hundreds of phones.

lm_attn_body gives each of its four waves the 64-key blocks w, w + 4, ... and merges the waves' (max, sum, output) through LDS, so an
encoder of at most 64 positions leaves waves 1-3 idle.  Here: the encoder with padding masks that end in every kind of block; sampled
decodes to 1024 tokens over a padded ~300-position encoder (the cross-attention's mask in later blocks); the sampling controls over 600
tokens; the longest greedy decode the config allows (max_position_embeddings = 3072); and greedy beam search over 200 - 400 tokens, whose
self-attention reads its keys through the ancestry table, against tests/lm_beam_numpy.py's driver (which reorders its caches instead).

Every exact-token assertion rests on a margin checked first: a sampling uniform is redrawn while it lies within U_MARGIN of a step of
its own CDF, and greedy / beam decisions need a score gap the test asserts.  The decode oracles start from the library's encoder states
(the encoder has its own test), so a token mismatch points at the decode."""
import os

import numpy as np
import pytest

import lm_beam_numpy as NB
from conftest import ROOT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

U_MARGIN = 1e-3          # distance of every sampling uniform from its CDF's steps
GREEDY_GAP = 1e-4        # best vs second score of every greedy choice
TIE_GAP = 1e-3           # a top-k boundary closer than this: the uniform must give the same token on either side of it
BEAM_GAP = 2e-4          # every selection of a beam search (NB.beam_step's "gap")
LOGIT_TOL = 2e-5
ES = {True: 1, False: 0, "never": 2}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def relmax(a, b):
    return float(np.abs(a - b).max() / max(1e-30, np.abs(b).max()))


def phones(B, L, seed):
    rng = np.random.default_rng(seed)
    phone = rng.integers(1, 108, size=(B, L)).astype(np.int64)
    tone = rng.integers(0, 12, size=(B, L)).astype(np.int64)
    spk = np.repeat(rng.integers(1, 324, size=B).astype(np.int64)[:, None], L, axis=1)
    return phone, tone, spk


def mask_of(lens, L):
    return (np.arange(L)[None, :] < np.asarray(lens)[:, None]).astype(np.int64)


@pytest.fixture(scope="module")
def lm_gpu():
    import yaml
    from text2semantic.utils import get_language_model
    args = yaml.safe_load(open(os.path.join(ROOT, "tests", "golden", "config_lm_like_reference.yaml")))
    return get_language_model(**args).to("cuda").eval()


@pytest.fixture(scope="module")
def wts(lm_gpu):
    return {k: v.detach().cpu().numpy().copy() for k, v in lm_gpu.state_dict().items()}


def with_eos_bias(w, cfg, bias):
    """the oracle's weights with `bias` added to the LM head's EOS bias"""
    if not bias:
        return w
    w = dict(w)
    b = w["semantic_decoder.cls.predictions.bias"].copy()
    b[cfg["sem_eos"]] += np.float32(bias)
    w["semantic_decoder.cls.predictions.bias"] = w["semantic_decoder.cls.predictions.decoder.bias"] = b
    return w


class EosBias:
    """the same bias on the device model for the duration of a block"""

    def __init__(self, m, bias):
        self.m, self.bias = m, float(bias)

    def _add(self, v):
        if v:
            with torch.no_grad():
                self.m.semantic_decoder.cls.predictions.bias[self.m.semantic_eos_token_id] += v
            self.m._native = None

    def __enter__(self):
        self._add(self.bias)

    def __exit__(self, *exc):
        self._add(-self.bias)


def oracle_decode(w, cfg, enc, enc_len, max_length, do_sample, top_k=5, top_p=1.0, temp=1.0, pen=1.0, ngram=0, seed=0):
    """oracle.roformer.generate's loop (cached decoder step, finished rows fed PAD) with the token choice of HF's processors
    (RepetitionPenalty -> NoRepeatNGram -> Temperature -> TopK -> TopP -> draw, oracle.roformer.pick_token_hf; greedy: argmax after the
    ban).  Each uniform comes from `seed`'s stream and is redrawn while it lies within U_MARGIN of a step of its own CDF, or while a nearly
    tied top-k boundary or nucleus cut, moved to its other side, would change the token.  Returns tokens
    [B, n], logits [n - 1, B, V], the uniforms [max_length - 1, B], the smallest uniform-to-step distance and the smallest score gap
    at a selection boundary (top-k: ranks k | k + 1 of the processed scores; greedy: best vs second)."""
    from oracle import roformer as R
    B, V = enc.shape[0], cfg["sem_vocab"]
    bos, eos, pad = cfg["sem_bos"], cfg["sem_eos"], cfg["sem_pad"]
    rng = np.random.default_rng(seed)
    kv = R.cross_kv(w, cfg, enc)
    caches = [dict() for _ in range(cfg["dec_layers"])]
    seq = np.full((B, max_length), pad, np.int64)
    seq[:, 0] = bos
    alive = np.ones(B, bool)
    U = np.full((max_length - 1, B), 0.5, np.float32)
    logits, udist, gap, n = [], np.inf, np.inf, max_length
    for step in range(max_length - 1):
        lg = R.decoder_step(w, cfg, seq[:, step], step, caches, kv, enc_len)
        logits.append(lg)
        for b in np.nonzero(alive)[0]:
            hist = seq[b, :step + 1]
            s = lg[b].copy()
            s[sorted(NB.ngram_banned(hist, ngram))] = -np.inf
            if not do_sample:
                top = np.sort(s)[-2:]
                gap = min(gap, float(top[1] - top[0]))
                tok = int(np.argmax(s))
            else:
                # the draws the uniform must agree with: this one, and where a selection boundary is nearly tied, the same draw with the
                # boundary on its other side (the k-th survivor of the top-k filter replaced by the (k + 1)-th; the nucleus mass moved by 1e-4)
                alts = [(s, top_p)]
                if top_k:
                    p = s.copy()
                    for t in set(hist.tolist()):
                        p[t] = p[t] * np.float32(pen) if p[t] < 0 else p[t] / np.float32(pen)
                    p = (p * np.float32(1.0 / temp)).astype(np.float32)
                    order = np.argsort(-p, kind="stable")
                    g = float(p[order[top_k - 1]] - p[order[top_k]])
                    gap = min(gap, g)
                    if g < TIE_GAP:
                        alt = s.copy()
                        alt[order[top_k - 1]] = -np.inf
                        alts.append((alt, top_p))
                if top_p < 1.0:
                    alts += [(s, top_p - 1e-4), (s, top_p + 1e-4)]
                for _ in range(1000):
                    u = np.float32(rng.random())
                    picks = [R.pick_token_hf(a, hist, top_k, tp, temp, pen, u, with_cdf=True) for a, tp in alts]
                    d = min(float(np.abs(c - u).min()) for _, c in picks)
                    if d >= U_MARGIN and len({t for t, _ in picks}) == 1:
                        break
                else:
                    raise AssertionError(f"no uniform {U_MARGIN} away from the CDF steps at step {step}, row {b}")
                tok = picks[0][0]
                U[step, b], udist = u, min(udist, d)
            seq[b, step + 1] = tok
            alive[b] = tok != eos
        if not alive.any():
            n = step + 2
            break
    return seq[:, :n], np.stack(logits), U, udist, gap


# ---- the encoder: lengths whose padding mask ends in every kind of 64-key block (block j belongs to wave j % 4) ----------------------------
ENC_CASES = {      # L -> per-row lengths (right-padded rows)
    "L65-len1-64-65": (65, [65, 1, 64]),                        # a single key; a full first block; one key in wave 1's block
    "L130-len63-97-130": (130, [63, 97, 130, 129]),             # inside block 0, mid block 1, two keys into wave 2's block
    "L257-len257-193-200": (257, [257, 193, 200, 256]),         # one key into block 4 (wave 0's second pass), wave 3's first key
    "L700-len450-513-700": (700, [450, 513, 700, 321]),         # inside blocks 7, 8, 10, 5: the waves' second and third passes
}


@pytest.mark.parametrize("case", list(ENC_CASES))
def test_encoder_long_ragged_vs_oracle(lm_gpu, wts, case, record_margin):
    """encode of a right-padded batch at L = 65 .. 700 against oracle.roformer.encoder_forward on the valid rows (2e-5), and every padded
    row bit for bit what the same row gives encoded alone, without padding"""
    from oracle import roformer as R
    m = lm_gpu
    L, lens = ENC_CASES[case]
    phone, tone, spk = phones(len(lens), L, L)
    enc = m.encode(dev(phone), dev(tone), dev(spk), attention_mask=dev(mask_of(lens, L))).cpu().numpy()
    ref = R.encoder_forward(wts, m.cfg, phone, tone, spk, np.array(lens))
    valid = mask_of(lens, L).astype(bool)
    record_margin(relmax(enc[valid], ref[valid]), LOGIT_TOL)
    for b, n in enumerate(lens):
        if n == L:
            continue
        alone = m.encode(dev(phone[b:b + 1, :n]), dev(tone[b:b + 1, :n]), dev(spk[b:b + 1, :n])).cpu().numpy()[0]
        assert np.array_equal(enc[b, :n], alone), (case, b, n, relmax(enc[b, :n], alone))


# ---- sampled decodes -----------------------------------------------------------------------------------------------------------------------
def run_sampled(m, w, enc, enc_len, max_length, do_sample, top_k, top_p, temp, pen, ngram, seed, record_margin, tag=""):
    """oracle first (uniforms with margins), then the library's decode with the same uniforms: tokens exact, per-step logits 2e-5"""
    cfg = m.cfg
    want, want_lg, U, udist, gap = oracle_decode(w, cfg, enc.cpu().numpy(), None if enc_len is None else enc_len.cpu().numpy(), max_length,
                                                 do_sample, top_k, top_p, temp, pen, ngram, seed)
    if do_sample:
        assert udist >= U_MARGIN, udist
    else:
        assert gap >= GREEDY_GAP, f"a greedy choice rests on a score gap of {gap:.2e}: choose other inputs"
    toks, lg = m.native().generate(enc, max_length, do_sample, top_k, top_p, temp, pen, dev(U) if do_sample else None, True, enc_len,
                                   no_repeat_ngram_size=ngram)
    toks, lg = toks.cpu().numpy(), lg.cpu().numpy()
    assert toks.shape == want.shape, (toks.shape, want.shape)
    bad = np.argwhere(toks != want)
    assert bad.size == 0, f"first token mismatch (row, position) {bad[0].tolist()}; smallest top-k gap {gap:.2e}"
    record_margin(relmax(lg, want_lg), LOGIT_TOL, tag)
    return toks, gap


@pytest.mark.parametrize("tag,eos_bias,seed", [("1024", 0.0, 1), ("1024-eos", 12.0, 2)])
def test_reference_call_1024_masked(lm_gpu, wts, monkeypatch, record_margin, tag, eos_bias, seed):
    """Roformer.generate as 22_infer_tts.py calls it (max_length 1024, top_k 5, top_p 1, temperature 1, no penalty), B = 4 over a right-padded
    300-position encoder (lengths 300, 211, 140, 65: the cross-attention's mask ends in blocks 4, 3, 2, 1), per-step logits and tokens
    against the oracle.  The EOS-biased variant: the rows stop at different steps, none on the host's 8-step poll, PAD after each EOS."""
    m = lm_gpu
    cfg = m.cfg
    L, lens, ML = 300, [300, 211, 140, 65], 1024
    phone, tone, spk = phones(len(lens), L, 300 + seed)
    mask = dev(mask_of(lens, L))
    w = with_eos_bias(wts, cfg, eos_bias)
    with EosBias(m, eos_bias):
        enc = m.encode(dev(phone), dev(tone), dev(spk), attention_mask=mask)
        want, want_lg, U, udist, gap = oracle_decode(w, cfg, enc.cpu().numpy(), np.array(lens), ML, True, seed=seed)
        assert udist >= U_MARGIN
        monkeypatch.setattr(torch, "rand", lambda *a, **k: dev(U))
        toks, lg = m.generate(dev(phone), dev(tone), attention_mask=mask, use_cache=None, max_length=ML, do_sample=True, temperature=1.0, top_k=5,
                              top_p=1.0, repetition_penalty=1.0, num_beams=1, no_repeat_ngram_size=0, early_stopping=True, spk_id=dev(spk),
                              end_gate_threshold=None, return_logits=True)
    toks, lg = toks.cpu().numpy(), lg.cpu().numpy()
    assert toks.shape == want.shape, (toks.shape, want.shape)
    bad = np.argwhere(toks != want)
    assert bad.size == 0, f"first token mismatch (row, position) {bad[0].tolist()}; smallest top-k gap {gap:.2e}"
    record_margin(relmax(lg, want_lg), LOGIT_TOL)
    if eos_bias:
        ends = [int(np.argmax(r == cfg["sem_eos"])) for r in toks]
        assert all((r == cfg["sem_eos"]).any() for r in toks) and len(set(ends)) == len(ends), ends
        assert max(ends) < ML - 1 and (max(ends) - 1) % 8 != 7, ends      # the last stop is not a poll step: the loop runs past it
        for r, e in zip(toks, ends):
            assert (r[e + 1:] == cfg["sem_pad"]).all()
    else:
        assert toks.shape == (len(lens), ML)


CONTROL_CASES = {      # tag -> (do_sample, top_k, top_p, temperature, penalty, n-gram size, seed)
    "full-vocab-topp0.8-temp1.3-pen1.2": (True, 0, 0.8, 1.3, 1.2, 0, 5),
    "topk8-pen1.2": (True, 8, 1.0, 1.0, 1.2, 0, 6),
    "sample-ngram2": (True, 5, 1.0, 1.0, 1.0, 2, 7),
    "greedy-ngram2": (False, 5, 1.0, 1.0, 1.0, 2, 8),
}


@pytest.mark.parametrize("case", list(CONTROL_CASES))
def test_sampling_controls_600_tokens(lm_gpu, wts, case, record_margin):
    """600 tokens, B = 3 over a right-padded 150-position encoder (lengths 150, 97, 64): the whole-vocabulary kernel (top_k 0) with its
    nucleus cut, temperature and a penalty that scans the whole history; the top-k kernel's penalty over 600 distinct-token marks; and the
    n-gram ban sampled and greedy -- tokens exact against pick_token_hf / NB.ngram_banned, per-step logits 2e-5"""
    m = lm_gpu
    do_sample, top_k, top_p, temp, pen, ngram, seed = CONTROL_CASES[case]
    L, lens = 150, [150, 97, 64]
    phone, tone, spk = phones(len(lens), L, 150 + seed)
    enc = m.encode(dev(phone), dev(tone), dev(spk), attention_mask=dev(mask_of(lens, L)))
    el = dev(np.array(lens, np.int32))
    run_sampled(m, wts, enc, el, 600, do_sample, top_k, top_p, temp, pen, ngram, seed, record_margin)


def test_greedy_decode_max_position_embeddings(lm_gpu, wts, record_margin):
    """the longest decode the config allows: greedy to max_length = max_position_embeddings (3072; rotary rows and cached keys to the end of
    the table), B = 2 over a right-padded 100-position encoder (lengths 100, 70); logits at every step, tokens exact"""
    m = lm_gpu
    L, lens = 100, [100, 70]
    phone, tone, spk = phones(len(lens), L, 3073)
    enc = m.encode(dev(phone), dev(tone), dev(spk), attention_mask=dev(mask_of(lens, L)))
    toks, _ = run_sampled(m, wts, enc, dev(np.array(lens, np.int32)), m.cfg["max_pos"], False, 1, 1.0, 1.0, 1.0, 0, 0, record_margin)
    assert toks.shape == (2, m.cfg["max_pos"])


# ---- greedy beam search against the numpy driver --------------------------------------------------------------------------------------
BEAM_CASES = {      # tag -> (K, max_length, encoder L, lengths, n-gram size, penalty, early_stopping, EOS bias, seed)
    "K4-len200-L300-ngram0-pen1-esTrue": (4, 200, 300, [300, 190], 0, 1.0, True, 0.0, 23),
    "K8-len200-L260-ngram2-pen1.2-esFalse": (8, 200, 260, [130, 260], 2, 1.2, False, 0.0, 21),
    "K4-len400-L300-ngram3-pen1.2-esNever": (4, 400, 300, [300, 257], 3, 1.2, "never", 0.0, 21),
    "K8-len400-L200-ngram0-pen1-esTrue": (8, 400, 200, [200, 66], 0, 1.0, True, 0.0, 21),
    "K4-len300-L150-ngram2-pen1-esTrue-eos": (4, 300, 150, [150, 97], 2, 1.0, True, 8.0, 27),
}


@pytest.mark.parametrize("case", list(BEAM_CASES))
def test_beam_search_long_vs_driver(lm_gpu, wts, case):
    """greedy beam search (self-attention keys through the ancestry table, past 64 and 256 cached positions; cross-attention over a padded
    encoder) token-exact against NB.generate_beam, which reorders its key / value caches by parent each step (HF's _reorder_cache)"""
    m = lm_gpu
    cfg = m.cfg
    K, ML, L, lens, ngram, pen, es, eos_bias, seed = BEAM_CASES[case]
    phone, tone, spk = phones(len(lens), L, 400 + seed)
    w = with_eos_bias(wts, cfg, eos_bias)
    with EosBias(m, eos_bias):
        enc = m.encode(dev(phone), dev(tone), dev(spk), attention_mask=dev(mask_of(lens, L)))
        want, gap = NB.generate_beam(w, cfg, enc.cpu().numpy(), K, ML, pen, ngram, ES[es], np.array(lens))
        assert gap >= BEAM_GAP, f"a beam selection rests on a score gap of {gap:.2e}: choose another seed"
        toks, _ = m.native().generate(enc, ML, False, 5, 1.0, 1.0, pen, None, False, dev(np.array(lens, np.int32)), num_beams=K,
                                      no_repeat_ngram_size=ngram, early_stopping=es)
    toks = toks.cpu().numpy()
    assert toks.shape == want.shape, (toks.shape, want.shape)
    bad = np.argwhere(toks != want)
    assert bad.size == 0, f"first token mismatch (item, position) {bad[0].tolist()}"
    if eos_bias:      # hypotheses finish at different lengths, PAD after the shorter one
        ends = [int(np.argmax(r == cfg["sem_eos"])) if (r == cfg["sem_eos"]).any() else None for r in toks]
        assert all(e is not None for e in ends) and len(set(ends)) == len(ends), ends
        for r, e in zip(toks, ends):
            assert (r[e + 1:] == cfg["sem_pad"]).all()
