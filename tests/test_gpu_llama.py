"""The text2semantic Llama on the GPU (csrc/llama.hip through Llama.generate / lds.native.Llama): the recorded cases of the reference's own
generate, rows of a ragged batch against the rows alone, the prefill against the cached step, the attention's boundaries against the numpy
restatement, indifference to the workspace's contents and to ids beyond the lengths, the stops, the limits, and infer_tts.py --lm_type llama."""
import ctypes as ct
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

import llama_numpy as LN

pytestmark = pytest.mark.gpu

LOGITS_TOL = 2e-5      # the project's LM logits bound
MIN_MARGIN = 1e-3
# attention-boundary runs against the restatement: weight seeds chosen on the CPU so that the restatement alone loses at most 10 % of its
# steps to a selection margin below MIN_MARGIN (seed 1 wide: none of 40, smallest margin 3.5e-3; seed 2 toy to 128 positions: none of 102, smallest 3.5e-3; wide seeds 0 and 2 lose steps)
WIDE_SEED, LONG_SEED = 1, 2


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


def build(config, K, seed, eos_row=None):
    """(module on the device, cfg, seeded state) -- the fixtures' weights when (config, K, seed) are theirs"""
    from lds import arch
    from text2semantic.llama.llama import Llama
    m = Llama(dict(config), semantic_kmeans_num=K, codebook_path="/nonexistent")
    state = arch.llama_init_state(m.cfg, seed)
    if eos_row is not None:
        state["llama.lm_head.weight"][m.cfg["eos"]] = eos_row
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    return m.cuda().eval(), m.cfg, state


@pytest.fixture(scope="module")
def toy(fx):
    t = dict(fx["toy"])
    return build(t, t.pop("semantic_kmeans_num"), int(fx["weight_seed"]))


@pytest.fixture(scope="module")
def toy_eos(fx):
    t = dict(fx["toy"])
    return build(t, t.pop("semantic_kmeans_num"), int(fx["weight_seed"]), eos_row=fx["eos_row"])


def case_kw(fx, tag):
    kw = dict(dict(temperature=1.0, top_k=5, top_p=1.0, repetition_penalty=1.0, no_repeat_ngram_size=0), **fx["cases"][tag])
    return kw


def row_alone(m, fx, tag, b, **extra):
    """row b of a case at B = 1 -> (tokens [n], logits [n, K + 3]) on the host"""
    u = fx.get(f"{tag}_r{b}_uniforms")
    ph = dev(fx[f"phone_r{b}"][None])
    toks, lg = m.generate(ph, torch.ones_like(ph), return_logits=True, uniforms=None if u is None else dev(u[:, None]), **dict(case_kw(fx, tag), **extra))
    return toks[0].cpu().numpy(), lg[:, 0].cpu().numpy()


def padded_batch(fx, order=(0, 1)):
    rows = [fx[f"phone_r{b}"] for b in order]
    L = max(len(r) for r in rows)
    ph = np.full((2, L), 77, dtype=np.int64)      # (whatever sits behind a row's length is never looked at)
    mask = np.zeros((2, L), dtype=np.int64)
    for i, r in enumerate(rows):
        ph[i, :len(r)] = r
        mask[i, :len(r)] = 1
    return dev(ph), dev(mask)


# ---- 1. the reference's recorded cases ----
@pytest.mark.parametrize("tag", ["greedy", "sample", "eos", "penalty"])
def test_fixture_cases(fx, toy, toy_eos, tag, record_margin):
    m, cfg, _ = toy_eos if tag == "eos" else toy
    for b in range(2):
        p = f"{tag}_r{b}_"
        assert float(fx[p + "margin"]) >= MIN_MARGIN      # no selection of the recorded run rests on a near-tie
        toks, lg = row_alone(m, fx, tag, b)
        ref = fx[p + "logits"]
        record_margin(relmax(lg[:len(ref)], ref), LOGITS_TOL, f"r{b}")
        assert np.array_equal(toks, fx[p + "tokens"])
        assert float(np.abs(lg).max()) <= 1.01 * float(fx[p + "absmax"]) + 1e-3


# ---- 2. a right-padded batch is its rows alone, bit for bit, in either order ----
@pytest.mark.parametrize("tag", ["greedy", "sample", "eos", "penalty"])
@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_batch_rows_equal_rows_alone(fx, toy, toy_eos, tag, order):
    m, cfg, _ = toy_eos if tag == "eos" else toy
    alone = [row_alone(m, fx, tag, b) for b in order]
    ph, mask = padded_batch(fx, order)
    u = None
    if f"{tag}_r0_uniforms" in fx:
        us = [fx[f"{tag}_r{b}_uniforms"] for b in order]
        u = np.zeros((max(len(x) for x in us), 2), dtype=np.float32)
        for i, x in enumerate(us):
            u[:len(x), i] = x
        u = dev(u)
    toks, lg = m.generate(ph, torch.ones_like(ph), attention_mask=mask, return_logits=True, uniforms=u, **case_kw(fx, tag))
    toks, lg = toks.cpu().numpy(), lg.cpu().numpy()
    pad = cfg["pad"] - cfg["shift"]
    assert toks.shape[1] == max(len(t) for t, _ in alone) and lg.shape[0] == toks.shape[1]
    for i, (t, l) in enumerate(alone):
        assert np.array_equal(toks[i, :len(t)], t) and (toks[i, len(t):] == pad).all()
        assert np.array_equal(lg[:len(t), i], l)      # bit for bit


# ---- 3. the prefill is the cached step: a call continued from a longer prefix gives the same tokens and logits ----
@pytest.mark.parametrize("tag", ["greedy", "sample"])
@pytest.mark.parametrize("n", [1, 9])
def test_prefill_equals_step(fx, toy, tag, n):
    m, cfg, _ = toy
    kw = case_kw(fx, tag)
    max_length = kw.pop("max_length")
    nat = m.native()
    ph, mask = padded_batch(fx)
    ids, lens = m.input_ids(ph, mask)
    u = None
    if tag == "sample":
        u = np.zeros((max_length - 1, 2), dtype=np.float32)
        for b in range(2):
            x = fx[f"sample_r{b}_uniforms"]
            u[:len(x), b] = x
    args = (max_length, kw["do_sample"], kw["top_k"], kw["top_p"], kw["temperature"], kw["repetition_penalty"])
    full, lg = nat.generate(ids, lens, *args, uniforms=None if u is None else dev(u), return_logits=True)
    gen = [int((full[b, lens[b]:] != cfg["pad"]).sum()) for b in range(2)]
    assert min(gen) > n + 1      # (both rows are still running n tokens in)
    # the prompt plus the first n generated ids of every row, right-padded with garbage
    wide = torch.full((2, max(lens) + n), 10 ** 9, dtype=torch.int64, device="cuda")
    for b in range(2):
        wide[b, :lens[b] + n] = full[b, :lens[b] + n]
    cont, lg2 = nat.generate(wide, [v + n for v in lens], *args, uniforms=None if u is None else dev(u[n:]), return_logits=True)
    assert torch.equal(cont, full)
    assert torch.equal(lg2, lg[n:n + lg2.shape[0]]) and lg2.shape[0] == lg.shape[0] - n


# ---- 4. attention boundaries against the restatement ----
def against_restatement(m, cfg, state, phones, max_length, record_margin):
    ids = LN.prompt_ids(cfg, phones)
    seq, ref, margins = LN.generate_row(state, cfg, m.inv_freq.numpy(), ids, max_length)
    ph = dev(np.asarray(phones, dtype=np.int64)[None])
    toks, lg = m.generate(ph, torch.ones_like(ph), max_length=max_length, do_sample=False, return_logits=True)
    toks, lg = toks[0].cpu().numpy(), lg[:, 0].cpu().numpy()
    # margins first: a step whose margin is below MIN_MARGIN ends the comparison there, and at most 10 % of the steps may be lost that way
    low = np.nonzero(margins < MIN_MARGIN)[0]
    n_ok = int(low[0]) if len(low) else len(margins)
    print(f"steps {len(margins)}, compared {n_ok}, smallest margin {margins.min():.3e}")
    assert n_ok >= 0.9 * len(margins)
    upto = min(n_ok + 1, len(margins))      # the logits of the low-margin step itself still follow the same history
    record_margin(relmax(lg[:upto], ref[:upto]), LOGITS_TOL)
    assert np.array_equal(toks[:n_ok], seq[len(ids):len(ids) + n_ok] - cfg["shift"])
    return toks


def test_reference_example_width_head_dim_192(record_margin):
    """the width of the reference's own example (llama.py:186-193) with 2 layers: head_dim 192 (three 64-channel groups per lane, pair
    blocks that straddle heads), kv_heads == heads, a vocabulary above 2048 columns; greedy, 40 tokens"""
    conf = dict(hidden_size=768, num_attention_heads=4, num_hidden_layers=2, intermediate_size=512, max_position_embeddings=256)
    m, cfg, state = build(conf, 2048, WIDE_SEED)
    assert cfg["head_dim"] == 192 and cfg["kv_heads"] == 4
    phones = (np.arange(15) * 7 % 107 + 1).astype(np.int64)
    toks = against_restatement(m, cfg, state, phones, 18 + 40, record_margin)
    assert len(toks) == 40 or toks[-1] == cfg["eos"] - cfg["shift"]


def test_toy_to_the_last_position(fx, record_margin):
    """max_length == max_position_embeddings: the last table row, key counts across the 64-key blocks of the attention's waves"""
    t = dict(fx["toy"])
    m, cfg, state = build(t, t.pop("semantic_kmeans_num"), LONG_SEED)
    toks = against_restatement(m, cfg, state, fx["phone_r0"], cfg["max_pos"], record_margin)
    assert len(toks) == cfg["max_pos"] - 26 or toks[-1] == cfg["eos"] - cfg["shift"]


# ---- 5. the workspace's contents and ids beyond the lengths change nothing; a repeat is bit-identical ----
def test_nan_workspace_garbage_ids_and_repeat(fx, toy):
    m, cfg, _ = toy
    nat = m.native()
    ph, mask = padded_batch(fx)
    ids, lens = m.input_ids(ph, mask)
    u = torch.rand(47, 2, generator=torch.Generator().manual_seed(3)).cuda()
    args = (48, True, 5, 0.9, 0.8, 1.2)
    t0, l0 = nat.generate(ids, lens, *args, uniforms=u, return_logits=True, no_repeat_ngram_size=3)
    t1, l1 = nat.generate(ids, lens, *args, uniforms=u, return_logits=True, no_repeat_ngram_size=3)
    assert torch.equal(t0, t1) and torch.equal(l0, l1)
    assert nat.ws.bufs
    for buf in nat.ws.bufs.values():
        buf.fill_(255)      # every float a NaN
    bad = ids.clone()
    junk = torch.tensor([-7, 10 ** 12, 3], device="cuda").repeat(ids.shape[1])
    for b in range(2):
        bad[b, lens[b]:] = junk[: ids.shape[1] - lens[b]]
    t2, l2 = nat.generate(bad, lens, *args, uniforms=u, return_logits=True, no_repeat_ngram_size=3)
    assert torch.equal(t0, t2) and torch.equal(l0, l2) and bool(torch.isfinite(l2).all())


# ---- 6. stops ----
def test_stops_at_max_length_and_at_eos(fx, toy, toy_eos):
    m, cfg, _ = toy
    ph, mask = padded_batch(fx)
    K = cfg["semantic_kmeans_num"]
    toks = m.generate(ph, torch.ones_like(ph), attention_mask=mask, max_length=40, do_sample=False)
    # rows of 26 and 18 prompt ids: 14 and 22 generated ids, the shorter row's tail padded with K + 2
    assert toks.shape == (2, 22) and bool((toks[0, 14:] == K + 2).all()) and bool((toks >= 0).all()) and bool((toks <= K + 2).all())
    me, _, _ = toy_eos
    te = me.generate(ph, torch.ones_like(ph), attention_mask=mask, max_length=48, do_sample=False).cpu().numpy()
    ends = [int(np.argmax(r == K + 1)) for r in te]
    assert all(te[b, ends[b]] == K + 1 for b in range(2)) and ends[0] != ends[1] and te.shape[1] == max(ends) + 1
    for b in range(2):
        assert (te[b, ends[b] + 1:] == K + 2).all()      # EOS kept, PAD after it


# ---- 7. every limit returns its code and enqueues nothing ----
def test_limits_return_codes_and_enqueue_nothing(toy):
    from lds import native
    m, cfg, _ = toy
    L = native.lib()
    nat = m.native()
    P, max_length = 9, 24
    nb = ct.c_size_t()
    assert L.lds_llama_workspace_bytes(nat.h, 2, P, max_length, ct.byref(nb)) == 0 and nb.value > 0
    need = nb.value

    def call(plen, B=2, ws_bytes=need, max_length=max_length, opts=None, uniforms=False):
        o = opts or native.LMDecodeOpts(0, 5, 1.0, 1.0, 1.0, 0, 1, 1)
        ids = torch.zeros(B, P, dtype=torch.int64, device="cuda")
        tokens = torch.full((B, max_length), 7, dtype=torch.int64, device="cuda")
        ws = torch.zeros(ws_bytes, dtype=torch.uint8, device="cuda")
        u = torch.zeros(max_length - 1, B, device="cuda") if uniforms else None
        n = ct.c_int(-5)
        pl = (ct.c_int32 * B)(*plen) if plen is not None else None
        rc = L.lds_llama_generate(nat.h, ids.data_ptr(), ct.cast(pl, ct.c_void_p) if pl else None, B, P, max_length, ct.byref(o),
                                  u.data_ptr() if u is not None else None, tokens.data_ptr(), None, ct.byref(n), ws.data_ptr(), ws.numel(), native._stream())
        torch.cuda.synchronize()
        assert bool((tokens == 7).all()) and n.value == -5 and not bool(ws.any()), "something ran"
        return rc

    assert call([9, 9], opts=native.LMDecodeOpts(0, 5, 1.0, 1.0, 1.0, 0, 2, 1)) == -1 and b"beam" in L.lds_last_error()
    assert call([0, 9]) == -1 and b"in_len[0]" in L.lds_last_error()
    assert call([9, 10]) == -1 and b"in_len[1]" in L.lds_last_error()
    assert call([3, 9], max_length=9) == -1 and b"in_len[1]" in L.lds_last_error() and b"max_length" in L.lds_last_error()
    assert call(None, max_length=9) == -1 and b"max_length" in L.lds_last_error()      # no lengths: P everywhere
    assert call([9, 9], max_length=cfg["max_pos"] + 1) == -1 and b"max_position_embeddings" in L.lds_last_error()
    assert call([9] * 65, B=65) == -1 and b"at most 64" in L.lds_last_error()
    assert L.lds_llama_workspace_bytes(nat.h, 65, P, max_length, ct.byref(nb)) == -1
    assert call([9, 9], opts=native.LMDecodeOpts(0, 5, 1.0, 1.0, 1.0, -1, 1, 1)) == -1 and b"no_repeat_ngram_size" in L.lds_last_error()
    assert call([9, 9], opts=native.LMDecodeOpts(1, 65, 1.0, 1.0, 1.0, 0, 1, 1), uniforms=True) == -1 and b"top_k" in L.lds_last_error()
    assert call([9, 9], opts=native.LMDecodeOpts(1, 5, 1.0, 1.0, 1.0, 0, 1, 1)) == -1 and b"uniforms" in L.lds_last_error()
    assert call([9, 9], ws_bytes=need - 256) == -2 and str(need).encode() in L.lds_last_error()
    # shapes the library refuses at create, before any tensor is looked at
    base = dict(hidden=96, heads=6, kv_heads=2, head_dim=16, inter=160, layers=2, vocab=172, max_pos=128, eps=1e-6, rope_theta=10000.0, first_free_id=108,
                bos=169, eos=170, pad=171)
    for bad, word in ((dict(head_dim=24), b"head_dim"), (dict(head_dim=272), b"head_dim"), (dict(head_dim=8), b"head_dim"), (dict(kv_heads=4), b"divide"),
                      (dict(vocab=108 + 8193, bos=200, eos=201, pad=202), b"columns")):
        c = native.LlamaCfg(**dict(base, **bad))
        h = ct.c_void_p()
        empty = (ct.c_void_p * 1)()
        assert L.lds_llama_create(ct.byref(c), 0, empty, empty, empty, ct.byref(h)) == -1 and word in L.lds_last_error() and not h.value


# ---- 8. the tool ----
def test_infer_tts_llama(tmp_path):
    sys.path.insert(0, ROOT)
    import infer_tts
    phones = tmp_path / "phones.npy"
    np.save(phones, np.stack([np.arange(19) * 7 % 107 + 1, np.arange(19) * 5 % 12]).astype(np.int64))
    torch.manual_seed(11)
    w = infer_tts.main(["--synthetic", "--lm_type", "llama", "--phones", str(phones), "--max_length", "40", "-s", "250", "-o", str(tmp_path / "a.npy")])
    assert w.ndim == 1 and w.shape[0] > 0 and np.isfinite(w).all()
    with pytest.raises(SystemExit):
        infer_tts.main(["--synthetic", "--lm_type", "llama", "--phones", str(phones), "--num_beams", "2", "-s", "250", "-o", str(tmp_path / "b.npy")])
