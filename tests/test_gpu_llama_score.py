"""Teacher-forced Llama scoring and prompted generation on the GPU (lds_llama_score / lds_llama_generate through Llama.score, score_ids and
generate): the reference forward's recorded cases, bit-identity with the cached decode and between a batch and its rows, the shape boundaries of
the attention, the row staging and the head's chunks against the numpy restatement, indifference to the workspace's contents and to whatever
sits behind the lengths, the limits, prompts that must reproduce the recorded decodes, and the tools."""
import ctypes as ct
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

import llama_score_numpy as LS

pytestmark = pytest.mark.gpu

LOGITS_TOL = 2e-5      # the project's LM logits bound; lp / loss: eps = 2 * LOGITS_TOL * absmax (log-sum-exp is 1-Lipschitz in the max norm)
WIDE_SEED = 1          # tests/test_gpu_llama.py's seed for the reference example's width
SHAPE_SEED = 3


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def relmax(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.fixture(scope="module")
def fx():
    f = dict(np.load(os.path.join(GOLDEN, "llama.npz")))
    f["cases"] = json.loads(bytes(f["cases_json"]).decode())
    f["toy"] = json.loads(bytes(f["toy_json"]).decode())
    return f


@pytest.fixture(scope="module")
def sx():
    return dict(np.load(os.path.join(GOLDEN, "llama_score.npz")))


def build(config, K, seed):
    from lds import arch
    from text2semantic.llama.llama import Llama
    m = Llama(dict(config), semantic_kmeans_num=K, codebook_path="/nonexistent")
    state = arch.llama_init_state(m.cfg, seed)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    return m.cuda().eval(), m.cfg, state


@pytest.fixture(scope="module")
def toy(fx):
    t = dict(fx["toy"])
    return build(t, t.pop("semantic_kmeans_num"), int(fx["weight_seed"]))


def pinned(logits, labels, eps):
    """position t is pinned when no other reference logit lies within eps of the label's (labels[t + 1] >= 0)"""
    out = np.zeros(len(labels) - 1, bool)
    for t in range(len(labels) - 1):
        y = int(labels[t + 1])
        if y >= 0:
            out[t] = np.abs(np.delete(logits[t], y) - logits[t, y]).min() > eps
    return out


def compare_row(lp, rank, logits, ref_lp, ref_rank, ref_logits, labels, record_margin, tag, min_pinned=0.9):
    """one row against a reference: logits relmax, lp within eps, ranks wherever the reference pins them (a condition on the REFERENCE, checked
    first: at least min_pinned of the counted positions)"""
    eps = 2 * LOGITS_TOL * float(np.abs(ref_logits).max())
    counted = np.asarray(labels[1:]) >= 0
    pin = pinned(ref_logits, labels, eps)
    err = float(np.abs(lp - ref_lp)[counted].max())
    print(f"{tag}: logits relmax {relmax(logits, ref_logits):.3e}, lp err {err:.3e} (eps {eps:.3e}), pinned {pin.sum()}/{counted.sum()}")
    assert pin.sum() >= min_pinned * counted.sum()
    record_margin(relmax(logits, ref_logits), LOGITS_TOL, tag + "-logits")
    record_margin(err, eps, tag + "-lp")
    assert np.array_equal(rank >= 0, counted) and np.array_equal(rank[pin], ref_rank[pin])
    assert (lp[~counted] == 0).all()
    return eps


# ---- 1. the reference forward's recorded cases ----
@pytest.mark.parametrize("case", ["greedy", "random"])
def test_score_fixture_cases(fx, sx, toy, case, record_margin):
    m, cfg, _ = toy
    shift = cfg["shift"]
    for b in range(2):
        p = f"{case}_r{b}_"
        ids, ref = sx[p + "ids"], sx[p + "logits"]
        # (i) the input_ids= path: labels default to input_ids
        r = m.score_ids(dev(ids[None]), return_logits=True)
        eps = compare_row(r.token_logprobs[0].cpu().numpy(), r.ranks[0].cpu().numpy(), r.logits[0].cpu().numpy(), sx[p + "lp"], sx[p + "rank"], ref, ids,
                          record_margin, f"r{b}")
        record_margin(abs(float(r.loss) - float(sx[p + "loss"])), eps, f"r{b}-loss")
        assert int(r.n_tokens) == len(ids) - 1
        assert abs(float(r.seq_logprob[0]) - float(sx[p + "lp"].sum())) < eps * (len(ids) - 1)
        # (ii) the phone / semantic path builds the same stream: the reference's training loss, and the per-token arrays at the semantic positions
        ph, sem = dev(fx[f"phone_r{b}"][None]), dev(sx[p + "semantic"][None])
        s = m.score(ph, torch.ones_like(ph), sem, append_eos=True, labels="stream", return_logits=True)
        at = len(fx[f"phone_r{b}"]) + 2
        T1 = sem.shape[1] + 1
        assert torch.equal(s.loss, r.loss) and torch.equal(s.n_tokens, r.n_tokens)
        assert torch.equal(s.token_logprobs[0], r.token_logprobs[0, at:at + T1]) and torch.equal(s.ranks[0], r.ranks[0, at:at + T1])
        assert s.logits.shape == (1, T1, cfg["vocab"] - shift) and torch.equal(s.logits[0], r.logits[0, at:at + T1, shift:])
        # labels None: the semantic targets (and the EOS) only
        o = m.score(ph, torch.ones_like(ph), sem, append_eos=True)
        assert torch.equal(o.token_logprobs, s.token_logprobs) and torch.equal(o.ranks, s.ranks) and int(o.n_tokens) == T1
        want = -float(sx[p + "lp"][at:at + T1].mean())
        assert abs(float(o.loss) - want) < eps


def test_score_fixture_batch_with_masked_labels(sx, toy, record_margin):
    m, cfg, _ = toy
    ids, mask, labels = sx["batch_ids"], sx["batch_mask"], sx["batch_labels"]
    r = m.score_ids(dev(ids), attention_mask=dev(mask), labels=dev(labels), return_logits=True)
    eps = 0.0
    for b in range(2):
        n = int(mask[b].sum())
        p = f"random_r{b}_"
        e = compare_row(r.token_logprobs[b, :n - 1].cpu().numpy(), r.ranks[b, :n - 1].cpu().numpy(), r.logits[b, :n].cpu().numpy(),
                        np.where(labels[b, 1:n] >= 0, sx[p + "lp"], 0), sx[p + "rank"], sx[p + "logits"], labels[b, :n], record_margin, f"r{b}")
        eps = max(eps, e)
        assert bool((r.ranks[b, n - 1:] == -1).all()) and bool((r.token_logprobs[b, n - 1:] == 0).all())
    record_margin(abs(float(r.loss) - float(sx["batch_loss"])), eps, "loss")
    assert int(r.n_tokens) == int(sx["batch_n"])


# ---- 2. the scoring pass is the cached decode, bit for bit; rows of a batch are the rows alone ----
def case_kw(fx, tag):
    return dict(dict(temperature=1.0, top_k=5, top_p=1.0, repetition_penalty=1.0, no_repeat_ngram_size=0), **fx["cases"][tag])


def decode_alone(m, fx, tag, b, **extra):
    u = fx.get(f"{tag}_r{b}_uniforms")
    ph = dev(fx[f"phone_r{b}"][None])
    toks, lg = m.generate(ph, torch.ones_like(ph), return_logits=True, uniforms=None if u is None else dev(u[:, None]), **dict(case_kw(fx, tag), **extra))
    return ph, toks, lg[:, 0]


def padded_phones(fx, order=(0, 1)):
    rows = [fx[f"phone_r{b}"] for b in order]
    L = max(len(r) for r in rows)
    ph, mask = np.full((2, L), 77, dtype=np.int64), np.zeros((2, L), dtype=np.int64)
    for i, r in enumerate(rows):
        ph[i, :len(r)] = r
        mask[i, :len(r)] = 1
    return dev(ph), dev(mask)


@pytest.mark.parametrize("tag", ["greedy", "sample"])
def test_score_logits_equal_the_decodes(fx, toy, tag):
    m, cfg, _ = toy
    alone = []
    for b in range(2):
        ph, toks, lg = decode_alone(m, fx, tag, b)
        assert np.array_equal(toks[0].cpu().numpy(), fx[f"{tag}_r{b}_tokens"])
        # (a sampled token may be the pad id K + 2 itself: the mask, not the row-end rule, says where these rows end)
        s = m.score(ph, torch.ones_like(ph), toks, semantic_attention_mask=torch.ones_like(toks), return_logits=True)
        assert s.logits.shape == (1,) + tuple(lg.shape) and torch.equal(s.logits[0], lg)      # bit for bit
        assert bool((s.ranks >= 0).all()) and int(s.n_tokens) == toks.shape[1]
        if tag == "greedy":      # a greedy token is the top of the columns 108 ..: at most the 108 phone columns can outrank it
            assert bool((s.ranks < 108).all())
        alone.append((toks[0], lg, s))
    # the padded two-row batch, in either order: the decode's logits again, and every row of the scoring batch equal to the row alone
    for order in ((0, 1), (1, 0)):
        ph, mask = padded_phones(fx, order)
        T = max(alone[b][0].shape[0] for b in order)
        sem = torch.full((2, T), cfg["pad"] - cfg["shift"], dtype=torch.int64, device="cuda")
        smask = torch.zeros_like(sem)
        for i, b in enumerate(order):
            sem[i, :alone[b][0].shape[0]] = alone[b][0]
            smask[i, :alone[b][0].shape[0]] = 1
        for kw in (dict(semantic_attention_mask=smask),) + ((dict(),) if tag == "greedy" else ()):      # the rows' ends from the mask, or from the pad ids
            s = m.score(ph, torch.ones_like(ph), sem, attention_mask=mask, return_logits=True, **kw)
            for i, b in enumerate(order):
                n = alone[b][0].shape[0]
                one = alone[b][2]
                assert torch.equal(s.logits[i, :n], alone[b][1]) and bool((s.logits[i, n:] == 0).all())
                assert torch.equal(s.token_logprobs[i, :n], one.token_logprobs[0]) and torch.equal(s.ranks[i, :n], one.ranks[0])
                assert bool((s.ranks[i, n:] == -1).all()) and abs(float(s.seq_logprob[i]) - float(one.seq_logprob[0])) < 1e-4
            assert int(s.n_tokens) == sum(int(a[2].n_tokens) for a in alone)


# ---- 3. shape boundaries against the restatement ----
@pytest.fixture(scope="module")
def shape_model(fx):
    """the toy widths with 320 positions, another seed; three seeded random streams and the restatement of the first over 257 positions"""
    t = dict(fx["toy"], max_position_embeddings=320)
    m, cfg, state = build(t, t.pop("semantic_kmeans_num"), SHAPE_SEED)
    rng = np.random.RandomState(11)
    streams = rng.randint(0, cfg["vocab"], size=(3, 257)).astype(np.int64)
    inv = m.inv_freq.numpy()
    lp, rank, loss, n, logits = LS.score_ids(state, cfg, inv, streams[:1])
    return m, cfg, state, inv, streams, dict(lp=lp[0], rank=rank[0], loss=loss, logits=logits[0])


def test_shape_257_rows_one_past_the_head_chunk(shape_model, record_margin):
    m, cfg, _, _, streams, ref = shape_model
    ids = dev(streams[:1])
    r = m.score_ids(ids, return_logits=True)
    eps = compare_row(r.token_logprobs[0].cpu().numpy(), r.ranks[0].cpu().numpy(), r.logits[0].cpu().numpy(), ref["lp"], ref["rank"], ref["logits"], streams[0],
                      record_margin, "S257")
    record_margin(abs(float(r.loss) - ref["loss"]), eps, "S257-loss")
    # without logits the head runs through the reused 256-row buffer (two chunks here): the same numbers
    q = m.score_ids(ids)
    assert q.logits is None and torch.equal(q.token_logprobs, r.token_logprobs) and torch.equal(q.ranks, r.ranks) and torch.equal(q.loss, r.loss)


@pytest.mark.parametrize("S", [2, 64, 65])
def test_shorter_streams_equal_prefixes_of_the_long_run(shape_model, S, record_margin):
    """S = 2: one counted position, one key; 64 / 65: the last lane of the attention's key block and the first key of the next wave"""
    m, cfg, _, _, streams, ref = shape_model
    full = m.score_ids(dev(streams[:1]), return_logits=True)
    r = m.score_ids(dev(streams[:1, :S]), return_logits=True)
    assert torch.equal(r.logits[0], full.logits[0, :S]) and torch.equal(r.token_logprobs[0], full.token_logprobs[0, :S - 1])
    assert torch.equal(r.ranks[0], full.ranks[0, :S - 1])
    record_margin(relmax(r.logits[0].cpu().numpy(), ref["logits"][:S]), LOGITS_TOL)
    eps = 2 * LOGITS_TOL * float(np.abs(ref["logits"]).max())
    assert abs(float(r.loss) + float(ref["lp"][:S - 1].astype(np.float64).mean())) < eps


def test_15_rows_not_a_multiple_of_the_staged_rows(shape_model, record_margin):
    """B * S = 15: the second 8-row tile of every linear is one row short; three different streams, one of them shorter"""
    m, cfg, state, inv, streams, _ = shape_model
    ids = streams[:, :5].copy()
    lens = [5, 3, 5]
    lp, rank, loss, n, logits = LS.score_ids(state, cfg, inv, ids, lens)
    r = m.score_ids(dev(ids), attention_mask=dev((np.arange(5)[None] < np.array(lens)[:, None]).astype(np.int64)), return_logits=True)
    eps = 0.0
    for b in range(3):
        labels = np.where(np.arange(5) < lens[b], ids[b], -100)
        eps = max(eps, compare_row(r.token_logprobs[b].cpu().numpy(), r.ranks[b].cpu().numpy(), r.logits[b, :lens[b]].cpu().numpy(), lp[b], rank[b],
                                   logits[b, :lens[b]], labels, record_margin, f"r{b}"))
    assert int(r.n_tokens) == n == 4 + 2 + 4 and abs(float(r.loss) - loss) < eps


def test_chunks_cross_the_rows_of_a_batch(shape_model):
    """B = 2, S = 257: 514 rows in three head chunks whose borders fall inside the rows; every row equals the row alone, bit for bit"""
    m, cfg, _, _, streams, _ = shape_model
    lens = torch.tensor([257, 130], dtype=torch.int32, device="cuda")
    nat = m.native()
    ids = dev(streams[:2])
    lp, rank, loss, n, _ = nat.score(ids, lens)
    a_lp, a_rank, _, a_n, _ = nat.score(ids[:1])
    b_lp, b_rank, _, b_n, _ = nat.score(ids[1:, :130].contiguous())
    assert torch.equal(lp[0], a_lp[0]) and torch.equal(rank[0], a_rank[0])
    assert torch.equal(lp[1, :129], b_lp[0]) and torch.equal(rank[1, :129], b_rank[0]) and bool((rank[1, 129:] == -1).all())
    assert int(n) == int(a_n) + int(b_n) == 256 + 129


def test_score_reference_example_width_head_dim_192(record_margin):
    """the width of the reference's own example (llama.py:186-193) with 2 layers: head_dim 192, kv_heads == heads, K 2048 -- a vocabulary of
    2159 columns, 108 + 2051: neither part of the head is a multiple of its 64-column blocks"""
    conf = dict(hidden_size=768, num_attention_heads=4, num_hidden_layers=2, intermediate_size=512, max_position_embeddings=256)
    m, cfg, state = build(conf, 2048, WIDE_SEED)
    assert cfg["head_dim"] == 192 and cfg["kv_heads"] == 4 and cfg["vocab"] == 2159
    phones = (np.arange(15) * 7 % 107 + 1).astype(np.int64)
    sem = np.random.RandomState(5).randint(0, 2048, 30).astype(np.int64)
    ids = LS.stream(cfg, phones, sem, append_eos=True)
    lp, rank, loss, n, logits = LS.score_ids(state, cfg, m.inv_freq.numpy(), ids[None])
    ph = dev(phones[None])
    s = m.score(ph, torch.ones_like(ph), dev(sem[None]), append_eos=True, labels="stream")
    r = m.score_ids(dev(ids[None]), return_logits=True)
    # 2159 columns within about +-2.5: the label's logit has a neighbour within eps = 1e-4 about twelve times as often as among the toy's 172
    # columns (1 to 2 % of the positions there), so the restatement pins fewer positions here: 40 of 48, computed on the CPU
    eps = compare_row(r.token_logprobs[0].cpu().numpy(), r.ranks[0].cpu().numpy(), r.logits[0].cpu().numpy(), lp[0], rank[0], logits[0], ids, record_margin, "wide",
                      min_pinned=0.75)
    record_margin(abs(float(r.loss) - loss), eps, "wide-loss")
    assert torch.equal(s.loss, r.loss) and torch.equal(s.token_logprobs[0], r.token_logprobs[0, 17:])


# ---- 4. the workspace's contents and whatever sits behind the lengths change nothing; a repeat is bit-identical ----
def test_nan_workspace_garbage_behind_the_lengths_and_repeat(sx, toy):
    m, cfg, _ = toy
    nat = m.native()
    ids, mask = dev(sx["batch_ids"]), sx["batch_mask"]
    lens = dev(mask.sum(1).astype(np.int32))
    labels = dev(sx["batch_labels"])
    first = nat.score(ids, lens, labels, return_logits=True)
    again = nat.score(ids, lens, labels, return_logits=True)
    assert all(torch.equal(a, b) for a, b in zip(first[:4], again[:4])) and torch.equal(first[4], again[4])
    assert nat.ws.bufs
    for buf in nat.ws.bufs.values():
        buf.fill_(255)      # every float a NaN
    bad_ids, bad_labels = ids.clone(), labels.clone()
    junk = torch.tensor([-100, 10 ** 9, -7], device="cuda").repeat(ids.shape[1])
    for b in range(2):
        n = int(mask[b].sum())
        bad_ids[b, n:] = junk[: ids.shape[1] - n]
        bad_labels[b, n:] = junk[1: 1 + ids.shape[1] - n]
    got = nat.score(bad_ids, lens, bad_labels, return_logits=True)
    assert all(torch.equal(a, b) for a, b in zip(first[:4], got[:4]))
    for b in range(2):      # the logits rows inside the lengths are the same bits (the rows behind them belong to the PAD filling either way)
        n = int(mask[b].sum())
        assert torch.equal(got[4][b, :n], first[4][b, :n])
    assert bool(torch.isfinite(got[4]).all()) and bool(torch.isfinite(got[2]))
    chunked = nat.score(bad_ids, lens, bad_labels)      # ... and through the reused chunk buffer
    assert all(torch.equal(a, b) for a, b in zip(first[:4], chunked[:4]))
    # nothing counted: NaN, 0 positions
    none = nat.score(ids, lens, torch.full_like(labels, -100))
    assert bool(torch.isnan(none[2])) and int(none[3]) == 0 and bool((none[1] == -1).all())


# ---- 5. every limit returns its code and enqueues nothing ----
def test_limits_return_codes_and_enqueue_nothing(toy):
    from lds import native
    m, cfg, _ = toy
    L = native.lib()
    nat = m.native()
    nb = ct.c_size_t()
    assert L.lds_llama_score_workspace_bytes(nat.h, 2, 24, ct.byref(nb)) == 0 and nb.value > 0
    need = nb.value

    def call(B, S, ws_bytes=need, n_ids=None):
        ids = torch.zeros(n_ids or B * S, dtype=torch.int64, device="cuda")
        out = torch.full((4096,), 7.0, device="cuda")      # logprobs, loss: never written by a refused call
        rk = torch.full((4096,), 7, dtype=torch.int32, device="cuda")
        ws = torch.zeros(ws_bytes, dtype=torch.uint8, device="cuda")
        rc = L.lds_llama_score(nat.h, ids.data_ptr(), None, None, B, S, out.data_ptr(), rk.data_ptr(), out[4000:].data_ptr(), rk[4000:].data_ptr(), None,
                               ws.data_ptr(), ws.numel(), native._stream())
        torch.cuda.synchronize()
        assert bool((out == 7).all()) and bool((rk == 7).all()) and not bool(ws.any()), "something ran"
        return rc

    assert call(2, 1, n_ids=8) == -1 and b"2 .." in L.lds_last_error()
    assert call(0, 24, n_ids=8) == -1 and b"B >= 1" in L.lds_last_error()
    assert call(2, cfg["max_pos"] + 1) == -1 and b"max_position_embeddings" in L.lds_last_error()
    assert call(1, 15001, n_ids=8) == -1 and b"15000" in L.lds_last_error()
    assert call(4097, 128, n_ids=8) == -1 and b"524280" in L.lds_last_error()      # 524416 rows
    assert call(2, 24, ws_bytes=need - 256) == -2 and str(need).encode() in L.lds_last_error()
    assert L.lds_llama_score_workspace_bytes(nat.h, 2, cfg["max_pos"] + 1, ct.byref(nb)) == -1
    assert L.lds_llama_score(nat.h, None, None, None, 2, 24, None, None, None, None, None, None, 0, None) == -1 and b"null" in L.lds_last_error()


# ---- 6. prompts ----
@pytest.mark.parametrize("n", [1, 9])
def test_prompt_reproduces_the_recorded_decodes(fx, toy, n):
    m, cfg, _ = toy
    K = cfg["semantic_kmeans_num"]
    for tag in ("greedy", "sample"):
        for b in range(2):
            ph, toks, lg = decode_alone(m, fx, tag, b)
            want = fx[f"{tag}_r{b}_tokens"]
            prompt = dev(np.concatenate([[K], want[:n]])[None])
            u = fx.get(f"{tag}_r{b}_uniforms")
            got, lg2 = m.generate(ph, torch.ones_like(ph), semantic_prompt=prompt, return_logits=True, uniforms=None if u is None else dev(u[n:, None]),
                                  **case_kw(fx, tag))
            assert np.array_equal(got[0].cpu().numpy(), want)      # the prompt's tokens in front, then exactly the recorded continuation
            assert torch.equal(lg2[:, 0], lg[n:])                  # the logits that chose the generated tokens, bit for bit
    # the prompt is looked at: another one gives another continuation
    ph = dev(fx["phone_r0"][None])
    other = m.generate(ph, torch.ones_like(ph), semantic_prompt=dev(np.array([[K, 3, 1, 4, 1, 5]])), **case_kw(fx, "greedy"))
    assert other[0, :5].tolist() == [3, 1, 4, 1, 5] and not np.array_equal(other[0].cpu().numpy(), fx["greedy_r0_tokens"])


@pytest.mark.parametrize("tag", ["greedy", "sample"])
def test_ragged_prompt_batch_equals_rows_alone(fx, toy, tag):
    """two rows with different phone lengths and different prompt lengths: each row equals that row run alone"""
    m, cfg, _ = toy
    K = cfg["semantic_kmeans_num"]
    kw = case_kw(fx, tag)
    np_ = (9, 4)      # prompt tokens per row (BOS not counted)
    ph, mask = padded_phones(fx)
    prompt = np.full((2, 10), 5, dtype=np.int64)      # (whatever sits behind a row's length is never looked at)
    pmask = np.zeros((2, 10), dtype=np.int64)
    alone, u = [], np.zeros((kw["max_length"] - 1, 2), dtype=np.float32)
    for b in range(2):
        rec = fx[f"{tag}_r{b}_tokens"]
        prompt[b, 0], prompt[b, 1:1 + np_[b]], pmask[b, :1 + np_[b]] = K, rec[:np_[b]], 1
        ub = fx.get(f"{tag}_r{b}_uniforms")
        if ub is not None:
            u[:len(ub) - np_[b], b] = ub[np_[b]:]
        p1 = dev(fx[f"phone_r{b}"][None])
        alone.append(m.generate(p1, torch.ones_like(p1), semantic_prompt=dev(prompt[b:b + 1, :1 + np_[b]]), return_logits=True,
                                uniforms=None if ub is None else dev(ub[np_[b]:, None]), **kw))
        assert np.array_equal(alone[b][0][0].cpu().numpy(), rec)
    toks, lg = m.generate(ph, torch.ones_like(ph), attention_mask=mask, semantic_prompt=dev(prompt), prompt_attention_mask=dev(pmask), return_logits=True,
                          uniforms=dev(u) if tag == "sample" else None, **kw)
    pad = cfg["pad"] - cfg["shift"]
    for b in range(2):
        t, l = alone[b]
        assert torch.equal(toks[b, :t.shape[1]], t[0]) and bool((toks[b, t.shape[1]:] == pad).all())
        assert torch.equal(lg[:l.shape[0], b], l[:, 0])


# ---- 7. the tools ----
def test_tools(tmp_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import infer_tts
    import validate_lm
    phones = tmp_path / "phones.npy"
    np.save(phones, np.stack([np.arange(19) * 7 % 107 + 1, np.arange(19) * 5 % 12]).astype(np.int64))
    np.save(tmp_path / "prompt.npy", (np.arange(6) * 131 % 4096).astype(np.int64))
    base = ["--synthetic", "--lm_type", "llama", "--phones", str(phones), "--max_length", "44", "-s", "250"]
    torch.manual_seed(11)
    w = infer_tts.main(base + ["--prompt_tokens", str(tmp_path / "prompt.npy"), "-o", str(tmp_path / "a.npy")])
    assert w.ndim == 1 and w.shape[0] > 0 and np.isfinite(w).all()
    torch.manual_seed(11)
    k = infer_tts.main(base + ["--prompt_tokens", str(tmp_path / "prompt.npy"), "--keep_prompt", "-o", str(tmp_path / "k.npy")])
    assert k.shape[0] > w.shape[0]      # the prompt's six tokens are synthesised too
    w = infer_tts.main(base + ["--candidates", "3", "-o", str(tmp_path / "c.npy")])
    assert w.ndim == 1 and w.shape[0] > 0 and np.isfinite(w).all()
    res = validate_lm.main(["--synthetic", "--lm_type", "llama", "--synthetic_items", "2", "--synthetic_tokens", "24", "-o", str(tmp_path / "v.json")])
    assert len(res["items"]) == 2 and res["items"][0]["tokens"] == 17 + 3 + 24 and res["items"][0]["semantic_tokens"] == 25
    for key in ("loss", "top5_acc", "semantic_loss", "semantic_top5_acc"):
        assert np.isfinite(res[key]) and all(np.isfinite(i[key]) for i in res["items"])
    assert res["loss"] > 0 and json.load(open(tmp_path / "v.json")) == res
