"""Teacher-forced LM scoring (Roformer.score / lds_lm_score) on a real MI355X: parity with the reference's prefix evaluation
(tests/golden/lm_score.npz), bit-identity with the cached decode, independence of batch neighbours / padding ids / workspace contents,
the shape boundaries of the causal attention and of the head's row chunk, the limits of the C entry, and the tools on top.

Bounds (a priori, none tuned): logits relmax < 2e-5 (the project's LM bound, test_gpu_frontend.py); a log-prob is
logit_y - logsumexp(logits) and log-sum-exp is 1-Lipschitz in the max norm, so lp and the loss move by at most
eps = 2 * 2e-5 * absmax(logits) (1.8e-3 at the fixture's abs-max 44); a rank may move only across reference logits within eps of the label's:
rank_lo <= rank <= rank_hi as recorded by the recipe, exact wherever the band is empty."""
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


def case_args(s, tag):
    """Roformer.score's keyword arguments for a fixture case"""
    sem, lab, sl = s[tag + "_semantic"], s[tag + "_labels"], s[tag + "_sem_len"]
    T = sem.shape[1]
    kw = dict(semantic=dev(sem), labels=dev(lab))
    if (sl < T).any():
        kw["attention_mask"] = dev((np.arange(T)[None] < sl[:, None]).astype(np.int64))
    if tag + "_enc_len" in s:
        kw["encoder_attention_mask"] = dev(s["ragged_mask"])
    return kw


# ---- 1. parity with the fixture ----
@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_score_vs_reference_prefix_evaluation(golden, lm_gpu, inputs, record_margin, tag):
    s, g = golden("lm_score.npz"), golden("roformer.npz")
    r = lm_gpu.score(inputs["phone"], inputs["tone"], spk_id=inputs["spk_id"], return_logits=True, **case_args(s, tag))
    eps = 2 * LOGITS_TOL * float(s[tag + "_absmax"])
    lp, rank, logits = r.token_logprobs.cpu().numpy().astype(np.float64), r.ranks.cpu().numpy(), r.logits.cpu().numpy()
    counted = s[tag + "_rank"] >= 0
    e_lp = float(np.abs(lp - s[tag + "_lp"]).max())
    e_loss = abs(float(r.loss) - float(s[tag + "_loss"]))
    e_seq = float(np.abs(r.seq_logprob.cpu().numpy() - s[tag + "_lp"].sum(1)).max())
    pinned = counted & (s[tag + "_rank_lo"] == s[tag + "_rank_hi"])
    m = {"eps": eps, "lp_abs_err": e_lp, "loss_abs_err": e_loss, "loss": float(r.loss), "n_counted": int(r.n_tokens), "ranks_pinned": int(pinned.sum()),
         "ranks_counted": int(counted.sum()), "ranks_equal_reference": int((rank == s[tag + "_rank"])[counted].sum()),
         "top5_acc": float((rank[counted] < 5).mean())}
    if tag == "a":
        want = g["greedy_logits"].transpose(1, 0, 2)
        m["logits_relmax"] = relmax(logits[:, : want.shape[1]], want)
    if tag == "b":
        m["logits_relmax"] = relmax(logits[0], s["b_logits_row0"])
    print("lm_score_margins", json.dumps({tag: m}))      # the measured margins (profiles/r14_lm_score_parity_margins.json is a copy of one run's)
    if "logits_relmax" in m:
        record_margin(m["logits_relmax"], LOGITS_TOL, "logits")
    assert int(r.n_tokens) == int(s[tag + "_n_counted"])
    assert np.array_equal(rank >= 0, counted) and (lp[~counted] == 0).all() and (rank[~counted] == -1).all()
    assert e_lp < eps and e_loss < eps, (e_lp, e_loss, eps)
    assert e_seq < eps * counted.sum(1).max(), e_seq
    assert (rank[counted] >= s[tag + "_rank_lo"][counted]).all() and (rank[counted] <= s[tag + "_rank_hi"][counted]).all()
    assert 2 * pinned.sum() >= counted.sum() and np.array_equal(rank[pinned], s[tag + "_rank"][pinned])
    if tag == "a":
        assert pinned.sum() == counted.sum() and m["top5_acc"] == 1.0


# ---- 2. bit-identity with the decode ----
@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("max_length", [24, 40])
@pytest.mark.parametrize("do_sample", [False, True])
def test_score_logits_equal_the_decode_bit_for_bit(golden, lm_gpu, inputs, do_sample, max_length, padded):
    g = golden("roformer.npz")
    mask = dev(g["ragged_mask"]) if padded else None
    torch.manual_seed(7)
    toks, dec = lm_gpu.generate(inputs["phone"], inputs["tone"], attention_mask=mask, max_length=max_length, do_sample=do_sample, temperature=1.0, top_k=5,
                                top_p=1.0, repetition_penalty=1.0, spk_id=inputs["spk_id"], return_logits=True)
    n = toks.shape[1]
    assert n >= 2 and dec.shape[0] == n - 1
    r = lm_gpu.score(inputs["phone"], inputs["tone"], toks, encoder_attention_mask=mask, spk_id=inputs["spk_id"], return_logits=True)
    for t in range(n - 1):
        assert torch.equal(r.logits[:, t], dec[t]), (t, float((r.logits[:, t] - dec[t]).abs().max()))
    if not do_sample and not bool((toks >= lm_gpu.semantic_eos_token_id).any()):      # the greedy decode chose the arg-max: every label has rank 0
        assert bool((r.ranks == 0).all())


# ---- 3. rows alone, padding ids, workspace contents, repeats ----
def test_rows_alone_padding_ids_and_workspace_have_no_effect(golden, lm_gpu, inputs):
    s = golden("lm_score.npz")
    kw = case_args(s, "c")
    base = lm_gpu.score(inputs["phone"], inputs["tone"], spk_id=inputs["spk_id"], return_logits=True, **kw)

    def same(r, logits=True):
        ok = all(torch.equal(getattr(r, k), getattr(base, k)) for k in ("token_logprobs", "ranks", "seq_logprob", "n_tokens"))
        ok = ok and (torch.equal(r.loss, base.loss) or bool(torch.isnan(r.loss) & torch.isnan(base.loss)))
        if logits:
            for b, n in enumerate(s["c_sem_len"]):
                ok = ok and torch.equal(r.logits[b, :n], base.logits[b, :n])
        return ok

    assert same(lm_gpu.score(inputs["phone"], inputs["tone"], spk_id=inputs["spk_id"], return_logits=True, **kw))       # a repeat
    # 10^9 instead of -100 at and beyond the lengths, in the ids and in the labels
    sl = s["c_sem_len"]
    beyond = np.arange(s["c_semantic"].shape[1])[None] >= sl[:, None]
    big = dict(kw, semantic=dev(np.where(beyond, 10 ** 9, s["c_semantic"])), labels=dev(np.where(beyond, 10 ** 9, s["c_labels"])))
    assert same(lm_gpu.score(inputs["phone"], inputs["tone"], spk_id=inputs["spk_id"], return_logits=True, **big))
    # a NaN-filled workspace (0xff bytes), with and without the logits (the chunk buffer)
    for buf in lm_gpu.native().ws.bufs.values():
        buf.fill_(255)
    assert same(lm_gpu.score(inputs["phone"], inputs["tone"], spk_id=inputs["spk_id"], return_logits=True, **kw))
    for buf in lm_gpu.native().ws.bufs.values():
        buf.fill_(255)
    assert same(lm_gpu.score(inputs["phone"], inputs["tone"], spk_id=inputs["spk_id"], **kw), logits=False)
    # every row alone, cropped to its own lengths
    n_counted = 0
    for b in range(2):
        Lb, Tb = int(s["c_enc_len"][b]), int(sl[b])
        one = lm_gpu.score(inputs["phone"][b:b + 1, :Lb].contiguous(), inputs["tone"][b:b + 1, :Lb].contiguous(), kw["semantic"][b:b + 1, :Tb].contiguous(),
                           labels=kw["labels"][b:b + 1, :Tb].contiguous(), spk_id=inputs["spk_id"][b:b + 1, :Lb].contiguous(), return_logits=True)
        assert torch.equal(one.token_logprobs[0], base.token_logprobs[b, : Tb - 1]) and torch.equal(one.ranks[0], base.ranks[b, : Tb - 1])
        assert torch.equal(one.logits[0], base.logits[b, :Tb]) and torch.equal(one.seq_logprob[0], base.seq_logprob[b])
        n_counted += int(one.n_tokens)
    assert n_counted == int(base.n_tokens)


# ---- 4. boundaries ----
@pytest.fixture(scope="module")
def long_case(lm_gpu, inputs):
    """T = 257 tokens per row and their logits, once; the shorter lengths are prefixes (causality: a prefix's logits do not change)"""
    rng = np.random.default_rng(3)
    sem = rng.integers(0, 4096, size=(2, 257)).astype(np.int64)
    sem[:, 0] = lm_gpu.semantic_bos_token_id
    r = lm_gpu.score(inputs["phone"], inputs["tone"], dev(sem), spk_id=inputs["spk_id"], return_logits=True)
    return sem, r


@pytest.mark.parametrize("T", [2, 64, 65, 257])
def test_attention_block_boundaries_vs_numpy(lm_gpu, inputs, long_case, T):
    """the attention's 64-key lane block and 256-key wave stride: T = 2, 64, 65, 257 against the numpy restatement (oracle.roformer's functions,
    causal over all positions) and, as prefixes of one sequence, bit for bit against each other"""
    import lm_score_numpy as N
    sem, full = long_case
    r = full if T == 257 else lm_gpu.score(inputs["phone"], inputs["tone"], dev(sem[:, :T]), spk_id=inputs["spk_id"], return_logits=True)
    assert torch.equal(r.logits, full.logits[:, :T]) and torch.equal(r.token_logprobs, full.token_logprobs[:, : T - 1])
    assert torch.equal(r.ranks, full.ranks[:, : T - 1])
    if T == 257:
        w = {k: v.detach().cpu().numpy() for k, v in lm_gpu.state_dict().items()}
        cfg = lm_gpu.cfg
        ph, tn, sp = (inputs[k].cpu().numpy() for k in ("phone", "tone", "spk_id"))
        logits, lp, rank, loss, n = N.score(w, cfg, ph, tn, sp, sem)
        got = r.logits.cpu().numpy()
        e = relmax(got, logits)
        eps = 2 * LOGITS_TOL * float(np.abs(logits).max())
        print("T 257 vs numpy: logits relmax", e, "lp err", float(np.abs(r.token_logprobs.cpu().numpy() - lp).max()), "eps", eps)
        assert e < LOGITS_TOL, e
        assert float(np.abs(r.token_logprobs.cpu().numpy() - lp).max()) < eps and abs(float(r.loss) - loss) < eps and int(r.n_tokens) == n


def test_head_row_chunk_crossed_by_one_row(lm_gpu, inputs, long_case):
    """B * T = 257: one row more than the head's 256-row chunk; without logits_out the rows pass through the reused chunk buffer"""
    sem, full = long_case
    for ret in (False, True):
        r = lm_gpu.score(inputs["phone"][:1], inputs["tone"][:1], dev(sem[:1]), spk_id=inputs["spk_id"][:1], return_logits=ret)
        assert torch.equal(r.token_logprobs[0], full.token_logprobs[0]) and torch.equal(r.ranks[0], full.ranks[0])
    both = lm_gpu.score(inputs["phone"], inputs["tone"], dev(sem), spk_id=inputs["spk_id"])      # 514 rows, no logits
    assert torch.equal(both.token_logprobs, full.token_logprobs) and torch.equal(both.ranks, full.ranks) and torch.equal(both.loss, full.loss)


def test_ignored_labels(golden, lm_gpu, inputs):
    s = golden("lm_score.npz")
    sem = dev(s["b_semantic"])
    base = lm_gpu.score(inputs["phone"], inputs["tone"], sem, spk_id=inputs["spk_id"])
    lab = s["b_semantic"].copy()
    lab[1] = -100
    r = lm_gpu.score(inputs["phone"], inputs["tone"], sem, labels=dev(lab), spk_id=inputs["spk_id"])
    T = lab.shape[1]
    assert int(r.n_tokens) == T - 1 and bool(torch.isfinite(r.loss)) and bool((r.ranks[1] == -1).all()) and bool((r.token_logprobs[1] == 0).all())
    assert torch.equal(r.token_logprobs[0], base.token_logprobs[0]) and float(r.seq_logprob[1]) == 0.0
    want = -float(base.token_logprobs[0].double().sum()) / (T - 1)
    assert abs(float(r.loss) - want) <= 1e-6 * abs(want)
    r = lm_gpu.score(inputs["phone"], inputs["tone"], sem, labels=dev(np.full_like(lab, -100)), spk_id=inputs["spk_id"])
    assert int(r.n_tokens) == 0 and bool(torch.isnan(r.loss)) and bool((r.ranks == -1).all())      # HF: mean over nothing = NaN


# ---- 5. limits: an error code, nothing enqueued ----
def test_limits_return_codes_and_enqueue_nothing(lm_gpu, inputs):
    from lds import native
    L = native.lib()
    m = lm_gpu.native()
    enc = lm_gpu.encode(inputs["phone"], inputs["tone"], inputs["spk_id"])
    B, Le, V, max_pos = 2, enc.shape[1], lm_gpu.cfg["sem_vocab"], lm_gpu.cfg["max_pos"]
    nb = ct.c_size_t()

    def call(T, Lenc=Le, ws_bytes=None, B=B):
        Ta = max(T, 2)
        sem = torch.zeros(B, Ta, dtype=torch.int64, device="cuda")
        lp = torch.full((B, Ta), 7.0, device="cuda")
        ranks = torch.full((B, Ta), 7, dtype=torch.int32, device="cuda")
        loss, n = torch.full((1,), 7.0, device="cuda"), torch.full((1,), 7, dtype=torch.int32, device="cuda")
        ws = torch.zeros(ws_bytes if ws_bytes is not None else 1 << 20, dtype=torch.uint8, device="cuda")
        rc = L.lds_lm_score(m.h, enc.data_ptr(), None, B, Lenc, sem.data_ptr(), None, None, T, lp.data_ptr(), ranks.data_ptr(), loss.data_ptr(), n.data_ptr(),
                            None, ws.data_ptr(), ws.numel(), native._stream())
        torch.cuda.synchronize()
        assert bool((lp == 7).all()) and bool((ranks == 7).all()) and float(loss) == 7.0 and int(n) == 7 and not bool(ws.any()), "something ran"
        return rc

    for T in (1, 0, max_pos + 1):
        assert L.lds_lm_score_workspace_bytes(m.h, B, Le, T, ct.byref(nb)) == -1
        assert call(T) == -1 and b"out of range" in L.lds_last_error()
    for Lenc in (0, max_pos + 1):
        assert L.lds_lm_score_workspace_bytes(m.h, B, Lenc, 8, ct.byref(nb)) == -1 and call(8, Lenc=Lenc) == -1
    assert call(8, B=0) == -1
    assert L.lds_lm_score_workspace_bytes(m.h, B, Le, 8, ct.byref(nb)) == 0 and nb.value > 0
    assert call(8, ws_bytes=nb.value - 256) == -2 and str(nb.value).encode() in L.lds_last_error()
    # the workspace holds no [B * T, V] logits: 4096 more rows cost less than their logits would (and 8 x 1024 rows less than their 134 MB)
    nb4 = ct.c_size_t()
    assert L.lds_lm_score_workspace_bytes(m.h, 8, Le, 1024, ct.byref(nb)) == 0 and L.lds_lm_score_workspace_bytes(m.h, 4, Le, 1024, ct.byref(nb4)) == 0
    assert nb.value - nb4.value < 4096 * V * 4 and nb.value < 8 * 1024 * V * 4
    with pytest.raises(ValueError):      # ids inside the lengths are validated by the Python layer (the library clamps)
        lm_gpu.score(inputs["phone"], inputs["tone"], torch.full((2, 8), V, dtype=torch.int64, device="cuda"), spk_id=inputs["spk_id"])


# ---- 6. the tools ----
def test_validate_lm_synthetic(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import validate_lm
    out = tmp_path / "val.json"
    res = validate_lm.main(["--synthetic", "--synthetic_items", "3", "--synthetic_tokens", "40", "-o", str(out)])
    assert len(res["items"]) == 3 and np.isfinite(res["loss"]) and 0.0 <= res["top5_acc"] <= 1.0
    assert res["loss"] == pytest.approx(np.mean([i["loss"] for i in res["items"]])) and json.load(open(out))["loss"] == res["loss"]
    # random weights: the loss sits near log(V) and certainly above log(5)
    assert res["loss"] > np.log(5.0)


def test_infer_tts_candidates(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import infer_tts
    phones = tmp_path / "phones.npy"
    np.save(phones, np.stack([np.arange(19) * 7 % 107 + 1, np.arange(19) * 5 % 12]).astype(np.int64))
    common = ["--synthetic", "--phones", str(phones), "--max_length", "24", "-s", "250"]
    # the synthetic LM with its EOS logit biased far down (as tools/time_lm.py does): every candidate runs to max_length, so the three have the
    # same number of generated tokens and the highest mean log-prob per token is the highest sequence log-prob
    real_lm = infer_tts.synthetic_lm

    def lm_without_eos(dev):
        m = real_lm(dev)
        with torch.no_grad():
            m.semantic_decoder.cls.predictions.bias[m.semantic_eos_token_id] -= 1.0e4
        return m
    monkeypatch.setattr(infer_tts, "synthetic_lm", lm_without_eos)
    picked = []
    real = infer_tts.pick_candidate
    monkeypatch.setattr(infer_tts, "pick_candidate", lambda *a, **k: picked.append(real(*a, **k)) or picked[-1])
    torch.manual_seed(11)
    infer_tts.main(common + ["--candidates", "3", "-o", str(tmp_path / "c3.npy")])
    best, mean_lp, result = picked[0]
    assert mean_lp.shape == (3,) and best == int(mean_lp.argmax()) and result.seq_logprob.shape == (3,)
    n_gen = result.ranks.ge(0).sum(1)
    assert torch.equal(mean_lp, result.seq_logprob / n_gen)
    assert n_gen.tolist() == [23, 23, 23] and best == int(result.seq_logprob.argmax()) and float(result.seq_logprob[best]) == float(result.seq_logprob.max())
    # --candidates 1 is today's path: tensor-identical to a run without the option (same seed, no scoring call)
    del picked[:]
    torch.manual_seed(11)
    w1 = infer_tts.main(common + ["--candidates", "1", "-o", str(tmp_path / "c1.npy")])
    torch.manual_seed(11)
    w0 = infer_tts.main(common + ["-o", str(tmp_path / "c0.npy")])
    assert not picked and np.array_equal(w1, w0)
