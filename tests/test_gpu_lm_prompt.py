"""Prompted LM generation (Roformer.generate(semantic_prompt=...) / lds_lm_generate_prompt) on a real MI355X: parity with the reference's
HF call started from input_ids= (tests/golden/lm_prompt.npz), bit-identity of a continuation with the unprompted decode it continues, of
every row of a ragged batch with that row alone, and of the prefill + first step with the scoring path; padding ids and workspace contents;
the stop rules; the limits of the C entry; the tools on top.

Bounds: tokens exact (every fixture case has a selection margin >= 1e-3, far above the logits' error); greedy row-0 logits relmax < 2e-5,
the project's LM bound (test_gpu_frontend.py).  Everything else is torch.equal."""
import ctypes as ct
import json
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LOGITS_TOL = 2e-5
CASES = ["greedy", "sample", "ngram", "penalty", "eos", "ragged_greedy", "ragged_sample"]
BASE = dict(do_sample=False, temperature=1.0, top_k=5, top_p=1.0, repetition_penalty=1.0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def relmax(a, b):
    return float(np.abs(a - b).max() / max(1e-30, np.abs(b).max()))


@pytest.fixture(scope="module")
def lm_gpu():
    import yaml
    from text2semantic.utils import get_language_model
    args = yaml.safe_load(open(os.path.join(ROOT, "tests", "golden", "config_lm_like_reference.yaml")))
    return get_language_model(**args).to("cuda").eval()


@pytest.fixture(scope="module")
def inputs(golden):
    g = golden("roformer.npz")
    return {k: dev(g[k]) for k in ("phone", "tone", "spk_id")}


class EosBias:
    """a bias on the LM head's EOS logit for the duration of a block"""

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


def pmask(plen, P):
    return dev((np.arange(P)[None] < np.asarray(plen)[:, None]).astype(np.int64))


def gen(m, inputs, prompt, plen=None, mask=None, rows=slice(None), uniforms=None, **kw):
    """generate with a prompt -> (tokens, logits); rows selects batch rows of the shared inputs"""
    prompt = prompt if torch.is_tensor(prompt) else dev(prompt)
    pm = None if plen is None else pmask(plen, prompt.shape[1])
    return m.generate(inputs["phone"][rows], inputs["tone"][rows], attention_mask=mask, spk_id=inputs["spk_id"][rows], return_logits=True,
                      semantic_prompt=prompt, prompt_attention_mask=pm, uniforms=uniforms, **dict(BASE, **kw))


def row_ends(m, toks, plen):
    """length of every row of a returned batch: up to its EOS behind the prompt, else the whole width"""
    out = []
    for b, p in enumerate(plen):
        hit = (toks[b, p:] == m.semantic_eos_token_id).nonzero()
        out.append(int(p + hit[0, 0] + 1) if hit.numel() else toks.shape[1])
    return out


def same_rows(m, a, b, plen):
    """two (tokens, logits) results agree on everything that is specified: the tokens, and row b's logits at its own steps"""
    if not torch.equal(a[0], b[0]):
        return False
    return all(torch.equal(a[1][: n - p, r], b[1][: n - p, r]) for r, (n, p) in enumerate(zip(row_ends(m, a[0], plen), plen)))


# ---- 1. parity with the fixture ----
@pytest.mark.parametrize("tag", CASES)
def test_generate_vs_reference(golden, lm_gpu, inputs, record_margin, tag):
    fx = golden("lm_prompt.npz")
    kw = json.loads(bytes(fx["cases_json"]).decode())[tag]
    assert float(fx[tag + "_margin"]) >= 1e-3
    plen = fx[tag + "_prompt_len"].tolist()
    ragged = tag.startswith("ragged")
    u = None
    if kw.get("do_sample"):
        u = np.zeros((kw["max_length"] - 1, 2), dtype=np.float32)
        u[: fx[tag + "_uniforms"].shape[0]] = fx[tag + "_uniforms"]
        u = dev(u)
    with EosBias(lm_gpu, fx["eos_bias"] if tag == "eos" else 0.0):
        toks, logits = gen(lm_gpu, inputs, fx[tag + "_prompt"], plen if ragged else None, dev(fx["ragged_mask"]) if ragged else None, uniforms=u, **kw)
    want = fx[tag + "_tokens"]
    assert tuple(toks.shape) == want.shape and np.array_equal(toks.cpu().numpy(), want), (toks.tolist(), want.tolist())
    if tag == "greedy":
        e = relmax(logits[:, 0].cpu().numpy(), fx["greedy_logits_row0"])
        record_margin(e, LOGITS_TOL, "logits")
        assert e < LOGITS_TOL, e


# ---- 2. a continuation is exact ----
@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("do_sample,max_length", [(False, 24), (True, 40)])
def test_continuation_equals_the_unprompted_decode(golden, lm_gpu, inputs, do_sample, max_length, padded):
    g = golden("roformer.npz")
    mask = dev(g["ragged_mask"]) if padded else None
    u = torch.rand(max_length - 1, 2, generator=torch.Generator().manual_seed(7)).cuda() if do_sample else None
    kw = dict(BASE, do_sample=do_sample, max_length=max_length)
    toks, dec = lm_gpu.generate(inputs["phone"], inputs["tone"], attention_mask=mask, spk_id=inputs["spk_id"], return_logits=True, uniforms=u, **kw)
    n = toks.shape[1]
    assert n > 11 and not bool((toks[:, :10] >= lm_gpu.semantic_bos_token_id)[:, 1:].any())
    for P in (1, 2, 8, 9, 10):      # the edges of the linears' 8-row tile in the prefill (P - 1 rows per item)
        t2, l2 = gen(lm_gpu, inputs, toks[:, :P].contiguous(), mask=mask, uniforms=u[P - 1:] if do_sample else None, do_sample=do_sample, max_length=max_length)
        assert torch.equal(t2, toks), P
        assert l2.shape[0] == n - P and torch.equal(l2, dec[P - 1:]), (P, float((l2 - dec[P - 1:]).abs().max()))


# ---- 3. every row of a ragged batch equals the row alone ----
@pytest.fixture(scope="module")
def ragged_case(golden):
    fx = golden("lm_prompt.npz")
    u = np.zeros((39, 2), dtype=np.float32)
    u[: fx["ragged_sample_uniforms"].shape[0]] = fx["ragged_sample_uniforms"]
    return dict(prompt=fx["ragged_sample_prompt"], plen=fx["ragged_sample_prompt_len"].tolist(), elen=fx["ragged_len"].tolist(), mask=fx["ragged_mask"], u=u)


@pytest.mark.parametrize("do_sample", [False, True])
def test_rows_alone_and_swapped(lm_gpu, inputs, ragged_case, do_sample):
    c = ragged_case
    kw = dict(do_sample=do_sample, max_length=40 if do_sample else 24, repetition_penalty=1.2)
    u = dev(c["u"])[: kw["max_length"] - 1] if do_sample else None
    toks, logits = gen(lm_gpu, inputs, c["prompt"], c["plen"], dev(c["mask"]), uniforms=u, **kw)
    ends = row_ends(lm_gpu, toks, c["plen"])
    assert max(ends) == toks.shape[1]
    alone = []
    for b in range(2):
        Lb, Pb = c["elen"][b], c["plen"][b]
        one = {k: v[b:b + 1, :Lb].contiguous() for k, v in inputs.items()}
        t1, l1 = gen(lm_gpu, one, c["prompt"][b:b + 1, :Pb], uniforms=u[:, b:b + 1] if do_sample else None, **kw)
        assert t1.shape[1] == ends[b] and torch.equal(t1[0], toks[b, : ends[b]]), b
        assert bool((toks[b, ends[b]:] == lm_gpu.semantic_pad_token_id).all())
        assert l1.shape[0] == ends[b] - Pb and torch.equal(l1[:, 0], logits[: ends[b] - Pb, b]), b
        alone.append((t1, l1))
    # the two rows swapped: the results swap
    sw = {k: v.flip(0).contiguous() for k, v in inputs.items()}
    t2, l2 = gen(lm_gpu, sw, c["prompt"][::-1].copy(), c["plen"][::-1], dev(c["mask"][::-1].copy()), uniforms=u.flip(1).contiguous() if do_sample else None, **kw)
    assert torch.equal(t2, toks.flip(0))
    for b in range(2):
        assert torch.equal(l2[: ends[b] - c["plen"][b], 1 - b], logits[: ends[b] - c["plen"][b], b])


@pytest.mark.parametrize("ngram", [0, 3])
def test_rows_alone_without_top_k_filter(lm_gpu, inputs, ragged_case, ngram):
    """top_k = None: the whole-vocabulary token choice (lm_sample_full_rows_kernel), with and without the n-gram ban; and as a continuation"""
    c = ragged_case
    kw = dict(do_sample=True, top_k=None, top_p=0.9, max_length=40, repetition_penalty=1.2, no_repeat_ngram_size=ngram)
    u = dev(c["u"])
    toks, logits = gen(lm_gpu, inputs, c["prompt"], c["plen"], dev(c["mask"]), uniforms=u, **kw)
    ends = row_ends(lm_gpu, toks, c["plen"])
    assert logits.shape[0] == max(e - p for e, p in zip(ends, c["plen"]))
    for b in range(2):
        Lb, Pb = c["elen"][b], c["plen"][b]
        one = {k: v[b:b + 1, :Lb].contiguous() for k, v in inputs.items()}
        t1, l1 = gen(lm_gpu, one, c["prompt"][b:b + 1, :Pb], uniforms=u[:, b:b + 1], **kw)
        assert t1.shape[1] == ends[b] and torch.equal(t1[0], toks[b, : ends[b]]) and torch.equal(l1[:, 0], logits[: ends[b] - Pb, b]), b
    # the unprompted run of the same options, continued from its first 9 tokens
    mask = dev(c["mask"])
    t0, l0 = lm_gpu.generate(inputs["phone"], inputs["tone"], attention_mask=mask, spk_id=inputs["spk_id"], return_logits=True, uniforms=u, **dict(BASE, **kw))
    assert not bool((t0[:, 1:9] >= lm_gpu.semantic_bos_token_id).any())
    t2, l2 = gen(lm_gpu, inputs, t0[:, :9].contiguous(), mask=mask, uniforms=u[8:], **kw)
    assert torch.equal(t2, t0) and torch.equal(l2, l0[8:])


def test_prompt_wider_than_its_longest_row(lm_gpu, inputs, ragged_case):
    """the library entry with P = 14 above the longest length 9 (Roformer.generate crops the prompt to the longest row first): the prompt is
    read with stride P, the prefill's ids with the stride of the longest row"""
    c = ragged_case
    kw = dict(do_sample=True, max_length=40, repetition_penalty=1.2)
    u = dev(c["u"])
    mask = dev(c["mask"])
    toks, logits = gen(lm_gpu, inputs, c["prompt"], c["plen"], mask, uniforms=u, **kw)
    wide = dev(np.concatenate([c["prompt"], np.full((2, 5), 10 ** 9, dtype=np.int64)], axis=1))
    enc_len = lm_gpu._mask_to_lengths(mask)
    enc = lm_gpu.encode(inputs["phone"], inputs["tone"], inputs["spk_id"], attention_mask=mask)
    t2, l2 = lm_gpu.native().generate_prompt(enc, wide, c["plen"], 40, True, 5, 1.0, 1.0, 1.2, u, True, enc_len)
    assert same_rows(lm_gpu, (t2, l2), (toks, logits), c["plen"]) and l2.shape == logits.shape


# ---- 4. the attention's 64-key lane block and 256-key wave stride ----
@pytest.fixture(scope="module")
def long_prompt(lm_gpu):
    rng = np.random.default_rng(3)
    sem = rng.integers(0, 4096, size=(2, 257)).astype(np.int64)
    sem[:, 0] = lm_gpu.semantic_bos_token_id
    return sem


@pytest.mark.parametrize("P", [64, 65, 256, 257])
def test_attention_boundaries_vs_scoring(lm_gpu, inputs, long_prompt, P):
    toks, logits = gen(lm_gpu, inputs, long_prompt[:, :P], max_length=P + 6)
    assert toks.shape[1] == P + 6 and logits.shape[0] == 6 and torch.equal(toks[:, :P], dev(long_prompt[:, :P]))
    r = lm_gpu.score(inputs["phone"], inputs["tone"], toks, spk_id=inputs["spk_id"], return_logits=True)
    for s in range(6):      # s = 0 ties the prefill and the first step to the scoring path, the rest the steps behind it
        assert torch.equal(logits[s], r.logits[:, P - 1 + s]), (s, float((logits[s] - r.logits[:, P - 1 + s]).abs().max()))


def test_attention_boundaries_ragged_mix(lm_gpu, inputs, long_prompt):
    plen = [65, 257]
    toks, logits = gen(lm_gpu, inputs, long_prompt, plen, max_length=263)
    assert toks.shape[1] == 263 and logits.shape[0] == 263 - 65
    assert not bool((toks[0, 65:] >= lm_gpu.semantic_eos_token_id).any()), "row 0 is expected to run to max_length with these weights"
    r = lm_gpu.score(inputs["phone"], inputs["tone"], toks, spk_id=inputs["spk_id"], return_logits=True)
    for b, p in enumerate(plen):
        n = row_ends(lm_gpu, toks, plen)[b]
        for s in range(n - p):
            assert torch.equal(logits[s, b], r.logits[b, p - 1 + s]), (b, s)


# ---- 5. padding ids and workspace contents ----
def test_padding_ids_and_workspace_contents_have_no_effect(lm_gpu, inputs, ragged_case):
    c = ragged_case
    kw = dict(do_sample=True, max_length=40, repetition_penalty=1.2, no_repeat_ngram_size=3)
    u = dev(c["u"])
    base = gen(lm_gpu, inputs, c["prompt"], c["plen"], dev(c["mask"]), uniforms=u, **kw)
    assert same_rows(lm_gpu, gen(lm_gpu, inputs, c["prompt"], c["plen"], dev(c["mask"]), uniforms=u, **kw), base, c["plen"])      # a repeat
    beyond = np.arange(c["prompt"].shape[1])[None] >= np.asarray(c["plen"])[:, None]
    big = np.where(beyond, 10 ** 9, c["prompt"])
    assert same_rows(lm_gpu, gen(lm_gpu, inputs, big, c["plen"], dev(c["mask"]), uniforms=u, **kw), base, c["plen"])
    for poisoned_prompt in (c["prompt"], big):
        for buf in lm_gpu.native().ws.bufs.values():
            buf.fill_(255)
        first = gen(lm_gpu, inputs, poisoned_prompt, c["plen"], dev(c["mask"]), uniforms=u, **kw)
        assert same_rows(lm_gpu, first, base, c["plen"])
        assert same_rows(lm_gpu, gen(lm_gpu, inputs, poisoned_prompt, c["plen"], dev(c["mask"]), uniforms=u, **kw), first, c["plen"])


# ---- 6. stop rules ----
def test_stop_at_max_length_and_at_eos(lm_gpu, inputs, ragged_case):
    c = ragged_case
    prompt = np.concatenate([c["prompt"], c["prompt"][:, 1:3]], axis=1)      # [2, 11]
    eos, pad = lm_gpu.semantic_eos_token_id, lm_gpu.semantic_pad_token_id

    def alone(b, Pb, **kw):
        return gen(lm_gpu, {k: v[b:b + 1].contiguous() for k, v in inputs.items()}, prompt[b:b + 1, :Pb], **kw)

    # a row one short of max_length generates exactly one token; its neighbour runs on
    plen = [11, 4]
    toks, logits = gen(lm_gpu, inputs, prompt, plen, max_length=12)
    assert toks.shape == (2, 12) and logits.shape[0] == 8
    for b in range(2):
        t1, l1 = alone(b, plen[b], max_length=12)
        assert torch.equal(t1[0], toks[b]) and torch.equal(l1[:, 0], logits[: 12 - plen[b], b])
    assert gen(lm_gpu, inputs, prompt, max_length=12)[0].shape == (2, 12)      # both rows one short: one step in all
    # an EOS bias between the two rows' needs: the first generated token of exactly one row is EOS
    r = lm_gpu.score(inputs["phone"], inputs["tone"], dev(prompt[:, :9]), spk_id=inputs["spk_id"], return_logits=True)
    need = (r.logits[:, 8].max(-1).values - r.logits[:, 8, eos]).tolist()      # what the EOS logit lacks to the arg-max at the first step
    assert abs(need[0] - need[1]) > 0.1, need
    first = int(np.argmin(need))
    with EosBias(lm_gpu, 0.5 * (need[0] + need[1])):
        toks, logits = gen(lm_gpu, inputs, prompt[:, :9], max_length=24)
        assert int(toks[first, 9]) == eos and bool((toks[first, 10:] == pad).all()) and int(toks[1 - first, 9]) != eos
        t1, l1 = alone(1 - first, 9, max_length=24)
        assert torch.equal(t1[0], toks[1 - first, : t1.shape[1]]) and torch.equal(l1[:, 0], logits[: t1.shape[1] - 9, 1 - first])
        t0, _ = alone(first, 9, max_length=24)
        assert t0.shape == (1, 10) and int(t0[0, 9]) == eos


# ---- 7. limits: an error code, nothing enqueued ----
def test_limits_return_codes_and_enqueue_nothing(lm_gpu, inputs):
    from lds import native
    L = native.lib()
    m = lm_gpu.native()
    enc = lm_gpu.encode(inputs["phone"], inputs["tone"], inputs["spk_id"])
    Le, max_length, P = enc.shape[1], 24, 9
    nb = ct.c_size_t()
    assert L.lds_lm_workspace_bytes_prompt(m.h, 2, Le, max_length, P, ct.byref(nb)) == 0 and nb.value > 0
    need = nb.value

    def call(plen, B=2, beams=1, ws_bytes=need, max_length=max_length):
        o = native.LMDecodeOpts(0, 5, 1.0, 1.0, 1.0, 0, beams, 1)
        prompt = torch.zeros(B, P, dtype=torch.int64, device="cuda")
        tokens = torch.full((B, max_length), 7, dtype=torch.int64, device="cuda")
        ws = torch.zeros(ws_bytes, dtype=torch.uint8, device="cuda")
        e = enc if B == 2 else enc[:1].expand(B, -1, -1).contiguous()
        n = ct.c_int(-5)
        pl = (ct.c_int32 * B)(*plen) if plen is not None else None
        rc = L.lds_lm_generate_prompt(m.h, e.data_ptr(), None, B, Le, max_length, ct.byref(o), prompt.data_ptr(), ct.cast(pl, ct.c_void_p) if pl else None, P,
                                      None, tokens.data_ptr(), None, ct.byref(n), ws.data_ptr(), ws.numel(), native._stream())
        torch.cuda.synchronize()
        assert bool((tokens == 7).all()) and n.value == -5 and not bool(ws.any()), "something ran"
        return rc

    assert call([3, 9], max_length=9) == -1 and b"prompt_len[1]" in L.lds_last_error() and b"max_length" in L.lds_last_error()
    assert call([8, 3], max_length=6) == -1 and b"prompt_len[0]" in L.lds_last_error()
    assert call(None, max_length=9) == -1 and b"max_length" in L.lds_last_error()      # no lengths: P everywhere
    assert call([0, 9]) == -1 and b"out of range" in L.lds_last_error()
    assert call([9, 10]) == -1 and b"out of range" in L.lds_last_error()
    assert call([9] * 65, B=65) == -1 and b"at most 64" in L.lds_last_error()
    assert L.lds_lm_workspace_bytes_prompt(m.h, 65, Le, max_length, P, ct.byref(nb)) == -1
    assert call([9, 9], beams=2) == -1 and b"beam" in L.lds_last_error()
    assert call([9, 9], ws_bytes=need - 256) == -2 and str(need).encode() in L.lds_last_error()
    # P = 1 needs exactly the unprompted workspace; a prompt adds its rows
    nb1 = ct.c_size_t()
    assert L.lds_lm_workspace_bytes_prompt(m.h, 2, Le, max_length, 1, ct.byref(nb)) == 0
    assert L.lds_lm_workspace_bytes_opts(m.h, 2, Le, max_length, 1, ct.byref(nb1)) == 0 and nb.value == nb1.value
    assert L.lds_lm_workspace_bytes_prompt(m.h, 2, Le, 600, 512, ct.byref(nb)) == 0 and L.lds_lm_workspace_bytes_opts(m.h, 2, Le, 600, 1, ct.byref(nb1)) == 0
    assert nb.value > nb1.value


# ---- 8. P = 1 through the new entry is the old entry ----
@pytest.mark.parametrize("do_sample", [False, True])
def test_bos_only_prompt_is_the_unprompted_decode(golden, lm_gpu, inputs, do_sample):
    g = golden("roformer.npz")
    mask = dev(g["ragged_mask"])
    u = torch.rand(39, 2, generator=torch.Generator().manual_seed(3)).cuda() if do_sample else None
    kw = dict(BASE, do_sample=do_sample, max_length=40, repetition_penalty=1.2)
    toks, dec = lm_gpu.generate(inputs["phone"], inputs["tone"], attention_mask=mask, spk_id=inputs["spk_id"], return_logits=True, uniforms=u, **kw)
    bos = torch.full((2, 1), lm_gpu.semantic_bos_token_id, dtype=torch.int64, device="cuda")
    t1, l1 = gen(lm_gpu, inputs, bos, mask=mask, uniforms=u, **dict(kw))
    assert torch.equal(t1, toks) and torch.equal(l1, dec)
    wide = torch.cat([bos, torch.full((2, 4), 10 ** 9, dtype=torch.int64, device="cuda")], 1)      # P = 5, every length 1
    t2, l2 = gen(lm_gpu, inputs, wide, [1, 1], mask=mask, uniforms=u, **dict(kw))
    assert torch.equal(t2, toks) and torch.equal(l2, dec)


# ---- 9. the tools ----
def test_infer_tts_prompt_options(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import infer_tts
    phones = tmp_path / "phones.npy"
    np.save(phones, np.stack([np.arange(19) * 7 % 107 + 1, np.arange(19) * 5 % 12]).astype(np.int64))
    ptok = tmp_path / "ptok.npy"
    np.save(ptok, (np.arange(6) * 37 % 4096).astype(np.int64))
    pph = tmp_path / "pph.npy"
    np.save(pph, np.stack([np.arange(5) * 3 % 107 + 1, np.arange(5) % 12]).astype(np.int64))
    common = ["--synthetic", "--phones", str(phones), "--max_length", "24", "-s", "250"]
    real_lm = infer_tts.synthetic_lm

    def lm_without_eos(dev_):      # every run goes to max_length: the lengths below are known
        m = real_lm(dev_)
        with torch.no_grad():
            m.semantic_decoder.cls.predictions.bias[m.semantic_eos_token_id] -= 1.0e4
        return m
    monkeypatch.setattr(infer_tts, "synthetic_lm", lm_without_eos)
    prompt = ["--prompt_tokens", str(ptok), "--prompt_phones", str(pph)]
    torch.manual_seed(11)
    w = infer_tts.main(common + prompt + ["-o", str(tmp_path / "a.npy")])
    torch.manual_seed(11)
    wk = infer_tts.main(common + prompt + ["--keep_prompt", "-o", str(tmp_path / "b.npy")])
    # 7 prompt tokens (BOS + 6) of max_length 24: 17 continuation tokens; with the prompt kept, 23 (BOS never reaches the codebook)
    assert w.shape[-1] * 23 == wk.shape[-1] * 17 and w.shape[-1] > 0
    picked = []
    real = infer_tts.pick_candidate
    monkeypatch.setattr(infer_tts, "pick_candidate", lambda *a, **k: picked.append(real(*a, **k)) or picked[-1])
    torch.manual_seed(11)
    infer_tts.main(common + prompt + ["--candidates", "3", "-o", str(tmp_path / "c.npy")])
    best, mean_lp, result = picked[0]
    assert result.ranks.ge(0).sum(1).tolist() == [17, 17, 17] and best == int(mean_lp.argmax())
    for bad in (["--prompt_tokens", str(ptok)], ["--keep_prompt"], ["--prompt_phones", str(pph)]):      # prompt options without --phones are refused
        with pytest.raises(SystemExit):
            infer_tts.main(["--synthetic", "-s", "250", "-o", str(tmp_path / "g.npy")] + bad)


def test_infer_tts_without_prompt_options_is_unchanged(tmp_path, monkeypatch):
    """without the prompt options the output is what it was before there were any: for the same seed, the waveform built the old way, step by
    step in main's order (pipeline, LM, generate without prompt keywords, BOS stripped, synthesize)"""
    sys.path.insert(0, ROOT)
    import infer_tts
    phones = tmp_path / "phones.npy"
    np.save(phones, np.stack([np.arange(19) * 7 % 107 + 1, np.arange(19) * 5 % 12]).astype(np.int64))
    common = ["--synthetic", "--phones", str(phones), "--max_length", "24", "-s", "250"]
    real_lm = infer_tts.synthetic_lm

    def lm_without_eos(dev_):
        m = real_lm(dev_)
        with torch.no_grad():
            m.semantic_decoder.cls.predictions.bias[m.semantic_eos_token_id] -= 1.0e4
        return m
    monkeypatch.setattr(infer_tts, "synthetic_lm", lm_without_eos)
    torch.manual_seed(11)
    w0 = infer_tts.main(common + ["-o", str(tmp_path / "d.npy")])
    torch.manual_seed(11)
    svc, codebook, _ = infer_tts.synthetic_pipeline("cuda", 256)
    lm = infer_tts.synthetic_lm("cuda")
    svc.model.decoder.denoise_fn.set_gemm_mode("f32")
    svc.model.decoder.denoise_fn.set_latency_mode(False)
    pt = dev(np.load(phones).astype(np.int64))
    tok = lm.generate(pt[0:1], pt[1:2], attention_mask=None, use_cache=None, max_length=24, do_sample=True, temperature=1.0, top_k=5, top_p=1.0,
                      repetition_penalty=1.0, num_beams=1, no_repeat_ngram_size=0, early_stopping=True, spk_id=torch.ones_like(pt[0:1]), end_gate_threshold=None)
    assert tok.shape == (1, 24) and not bool((tok[:, 1:] >= lm.semantic_eos_token_id).any())
    _, _, old = infer_tts.synthesize(svc, codebook, tok[:, 1:].clamp(max=codebook.shape[0] - 1), 1, 250, "dpm-solver", None)
    assert np.array_equal(w0, old[0, 0].cpu().numpy())
    # and an empty prompt (BOS alone) is no prompt: the same tokens through the unprompted launches, the same waveform
    empty = tmp_path / "empty.npy"
    np.save(empty, np.zeros(0, dtype=np.int64))
    torch.manual_seed(11)
    we = infer_tts.main(common + ["--prompt_tokens", str(empty), "-o", str(tmp_path / "e.npy")])
    assert np.array_equal(w0, we) and w0.shape[-1] > 0


def test_text2semantic_rows_carries_per_row_prompts(monkeypatch):
    sys.path.insert(0, ROOT)
    import infer_tts
    lm = infer_tts.synthetic_lm("cuda")
    with torch.no_grad():
        lm.semantic_decoder.cls.predictions.bias[lm.semantic_eos_token_id] -= 1.0e4      # every row runs to max_length
    ph = dev((np.arange(2 * 19).reshape(2, 19) * 7 % 107 + 1).astype(np.int64))
    tn = dev((np.arange(2 * 19).reshape(2, 19) * 5 % 12).astype(np.int64))
    p0 = dev((np.arange(6) * 37 % 4096).astype(np.int64))
    u = torch.rand(23, 2, generator=torch.Generator().manual_seed(5)).cuda()
    monkeypatch.setattr(torch, "rand", lambda *a, **k: u)
    rows = infer_tts.text2semantic_rows(lm, ph, tn, max_length=24, phone_lengths=[19, 12], prompt_rows=[p0, None])
    kept = infer_tts.text2semantic_rows(lm, ph, tn, max_length=24, phone_lengths=[19, 12], prompt_rows=[p0, None], keep_prompt=True)
    assert [int(r.numel()) for r in rows] == [17, 23] and [int(r.numel()) for r in kept] == [23, 23]
    assert torch.equal(kept[0][:6], p0) and torch.equal(kept[0][6:], rows[0]) and torch.equal(kept[1], rows[1])
    # row 1 has no prompt: it is the row of the unprompted batch (same uniforms: its s-th token uses uniforms[s][1] either way)
    plain = infer_tts.text2semantic_rows(lm, ph, tn, max_length=24, phone_lengths=[19, 12])
    assert torch.equal(plain[1], rows[1])


def test_infer_tts_prompt_audio(tmp_path):
    sys.path.insert(0, ROOT)
    import infer_tts
    phones, clip = tmp_path / "phones.npy", tmp_path / "clip.npy"
    np.save(phones, np.stack([np.arange(19) * 7 % 107 + 1, np.arange(19) * 5 % 12]).astype(np.int64))
    t = np.arange(16000, dtype=np.float32) / 16000
    np.save(clip, (0.3 * np.sin(2 * np.pi * 220 * t) + 0.1 * np.sin(2 * np.pi * 557 * t)).astype(np.float32))      # 1 s at 16 kHz: 50 unit frames
    args = ["--synthetic", "--phones", str(phones), "--max_length", "64", "-s", "250", "--prompt_audio", str(clip), "--prompt_encoder_layers", "1"]
    torch.manual_seed(3)
    w = infer_tts.main(args + ["-o", str(tmp_path / "a.npy")])
    torch.manual_seed(3)
    wk = infer_tts.main(args + ["--keep_prompt", "-o", str(tmp_path / "b.npy")])
    # 50 prompt tokens + BOS of max_length 64 (the synthetic LM's EOS is not biased here, so a row may stop early: at most 13 / 63 tokens)
    assert 0 < w.shape[-1] < wk.shape[-1] and (wk.shape[-1] - w.shape[-1]) * 13 >= 50 * w.shape[-1]
