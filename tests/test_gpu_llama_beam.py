"""The Llama's greedy beam search on the GPU (lds_llama_generate_beam through Llama.generate / lds.native.Llama): the cases the reference's own
generate recorded (tests/golden/llama_beam.npz), rows of a ragged batch against the rows alone, the beam step kernel against the numpy step
(tests/llama_beam_numpy.py), the beam attention against the plain attention on a physically gathered cache, whole decodes against the
restatement at the reference example's width and up to the last position, indifference to the workspace's contents, to ids beyond the lengths
and to the poll interval, and the limits."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import llama_beam_numpy as LB
import llama_numpy as LN

pytestmark = pytest.mark.gpu

MIN_MARGIN = 1e-3
ES = {True: 1, False: 0, "never": 2}
# whole decodes against the restatement: weight seeds chosen on the CPU so that the restatement's own margin is at least MIN_MARGIN at EVERY
# selection of the run (the test asserts it first; no step is skipped)
# (wide: seed 5, four beams, early_stopping True: 24 steps, smallest margin 1.8e-3; toy to 128 positions: seed 84, three beams, early_stopping False:
# 102 steps, smallest margin 1.2e-3; the seeds before them fall below 1e-3 somewhere)
WIDE_SEED, LONG_SEED = 5, 84
CASE_TAGS = ["beam3", "beam4_open", "beam2_never", "beam4_penalty", "eos", "prompt"]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def fx():
    f = dict(np.load(os.path.join(GOLDEN, "llama_beam.npz")))
    f["cases"] = json.loads(bytes(f["cases_json"]).decode())
    f["toy"] = json.loads(bytes(f["toy_json"]).decode())
    return f


def build(config, K, seed, eos_row=None):
    from lds import arch
    from text2semantic.llama.llama import Llama
    m = Llama(dict(config), semantic_kmeans_num=K, codebook_path="/nonexistent")
    state = arch.llama_init_state(m.cfg, seed)
    if eos_row is not None:
        state["llama.lm_head.weight"][m.cfg["eos"]] = eos_row
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    return m.cuda().eval(), m.cfg, state


_models = {}


def case_model(fx, tag):
    """the case's model (its own weight seed; the "eos" case's head row), built once"""
    if tag not in _models:
        t = dict(fx["toy"])
        _models[tag] = build(t, t.pop("semantic_kmeans_num"), int(fx[tag + "_weight_seed"]), fx["eos_row"] if tag == "eos" else None)
    return _models[tag]


def case_kw(fx, tag):
    return dict(dict(max_length=fx["cases"]["max_length"], do_sample=False), **fx["cases"][tag])


def run_rows(m, fx, tag, rows, **extra):
    """the rows of a case as one right-padded batch (one row: alone, un-padded) -> tokens [len(rows), n] on the host"""
    phones = [fx[f"phone_r{b}"] for b in rows]
    L = max(len(p) for p in phones)
    ph = np.full((len(rows), L), 77, dtype=np.int64)      # (whatever sits behind a row's length is never looked at)
    mask = np.zeros((len(rows), L), dtype=np.int64)
    for i, p in enumerate(phones):
        ph[i, :len(p)], mask[i, :len(p)] = p, 1
    kw = dict(case_kw(fx, tag), **extra)
    if tag == "prompt" or "prompt_rows" in kw:
        pr = kw.pop("prompt_rows", None) or [fx[f"prompt_r{b}"] for b in rows]
        P = max(len(p) for p in pr)
        sp = np.full((len(rows), P), 5, dtype=np.int64)
        pm = np.zeros((len(rows), P), dtype=np.int64)
        for i, p in enumerate(pr):
            sp[i, :len(p)], pm[i, :len(p)] = p, 1
        kw.update(semantic_prompt=dev(sp), prompt_attention_mask=dev(pm))
    return m.generate(dev(ph), dev(ph), attention_mask=dev(mask), **kw).cpu().numpy()


# ---- 1. the reference's recorded cases ----
@pytest.mark.parametrize("tag", CASE_TAGS)
def test_fixture_cases(fx, tag):
    m, cfg, _ = case_model(fx, tag)
    for b in range(2):
        assert float(fx[f"{tag}_r{b}_margin"]) >= MIN_MARGIN      # no selection of the recorded run rests on a near-tie
        toks = run_rows(m, fx, tag, [b])[0]
        want = fx[f"{tag}_r{b}_tokens"]
        if tag == "prompt":      # the returned row begins with the prompt's tokens
            want = np.concatenate([fx[f"prompt_r{b}"][1:], want])
        assert np.array_equal(toks, want), (b, toks.tolist(), want.tolist())


# ---- 2. a right-padded batch is its rows alone, in either order; a prompted row beside an unprompted one ----
@pytest.mark.parametrize("tag", CASE_TAGS)
@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_batch_rows_equal_rows_alone(fx, tag, order):
    m, cfg, _ = case_model(fx, tag)
    alone = [run_rows(m, fx, tag, [b])[0] for b in order]
    batch = run_rows(m, fx, tag, list(order))
    assert batch.shape[1] == max(len(a) for a in alone)
    for i, a in enumerate(alone):
        assert np.array_equal(batch[i, :len(a)], a), (i, batch[i].tolist(), a.tolist())
        assert (batch[i, len(a):] == cfg["semantic_kmeans_num"] + 2).all()


@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_prompted_row_beside_an_unprompted_one(fx, order):
    m, cfg, _ = case_model(fx, "prompt")
    K = cfg["semantic_kmeans_num"]
    prompts = {order[0]: fx[f"prompt_r{order[0]}"], order[1]: np.array([K], dtype=np.int64)}      # the second row: the semantic BOS alone
    alone = [run_rows(m, fx, "prompt", [b], prompt_rows=[prompts[b]])[0] for b in order]
    batch = run_rows(m, fx, "prompt", list(order), prompt_rows=[prompts[b] for b in order])
    for i, a in enumerate(alone):
        assert np.array_equal(batch[i, :len(a)], a), (i, batch[i].tolist(), a.tolist())
        assert (batch[i, len(a):] == K + 2).all()
    # a prompt of the BOS alone is no prompt
    ph = dev(fx[f"phone_r{order[1]}"][None])
    assert np.array_equal(alone[1], m.generate(ph, ph, **case_kw(fx, "prompt")).cpu().numpy()[0])


# ---- 3. the step kernel against the numpy step ----
def run_kernel_step(logits, K, step, max_length, eos, pen, ngram, es, first_free, plen, ended, state, unsat):
    from lds import native
    run_seq, run_score, fin_seq, fin_score, fin_flag, fin_len = state
    R, B = logits.shape[0], len(plen)
    pad = int(run_seq[0, -1])
    ins = [dev(a) for a in (logits, run_seq, run_score, fin_seq, fin_score, fin_flag.astype(np.int32), fin_len.astype(np.int32), unsat.astype(np.int32))]
    outs = dict(run_seq=torch.full_like(ins[1], pad), run_score=torch.zeros_like(ins[2]), parent=torch.zeros(R, dtype=torch.int32, device="cuda"),
                fin_seq=torch.full_like(ins[3], pad), fin_score=torch.zeros_like(ins[4]), fin_flag=torch.zeros_like(ins[5]),
                fin_len=torch.zeros_like(ins[6]), unsat=torch.zeros_like(ins[7]), ended=torch.full((B,), -3, dtype=torch.int32, device="cuda"),
                flags=torch.zeros(1, dtype=torch.int32, device="cuda"))
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    pl, en = (C.c_int32 * B)(*[int(v) for v in plen]), (C.c_int32 * B)(*[int(v) for v in ended])
    native.check(native.lib().lds_test_llama_beam_step(
        p(ins[0]), B, K, logits.shape[1], step, max_length, eos, C.c_float(pen), ngram, es, first_free, pl, en, *(p(t) for t in ins[1:]),
        p(outs["run_seq"]), p(outs["run_score"]), p(outs["parent"]), p(outs["fin_seq"]), p(outs["fin_score"]), p(outs["fin_flag"]),
        p(outs["fin_len"]), p(outs["unsat"]), p(outs["ended"]), p(outs["flags"]), native._stream()))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in outs.items()}


STEP_CASES = [      # (K, V, step, max_length, prompt lengths, ended, rep_pen, ngram, early_stopping, finished share, EOS boost)
    (2, 172, 0, 48, (26, 18, 1), (0, 0, 1), 1.0, 0, 1, 0.0, None),
    (8, 172, 9, 48, (26, 18, 30), (0, 0, 1), 1.2, 3, 1, 0.3, "top"),
    (2, 2305, 7, 60, (18, 26, 40), (0, 0, 1), 1.3, 2, 0, 0.5, "mid"),
    (8, 2305, 12, 39, (26, 18, 5), (0, 0, 1), 1.0, 0, 2, 0.4, None),          # the first item is at max_length: 26 + 12 + 1
    (2, 4352, 20, 80, (26, 59, 44), (0, 0, 1), 1.1, 1, 1, 1.0, "top"),        # every slot finished; the second item at max_length
    (8, 4352, 5, 64, (18, 26, 33), (0, 0, 1), 1.2, 2, 0, 0.3, "mid"),
    (8, 4352, 300, 400, (61, 26, 90), (0, 1, 0), 1.2, 3, 1, 0.3, "mid"),      # long histories; the frozen item in the middle
]


@pytest.mark.parametrize("case", range(len(STEP_CASES)))
def test_beam_step_kernel_vs_numpy(case):
    """V = 172, 2305 (the last size of the 36-values-per-lane form + 1) and 4352 (the limit), 2 and 8 beams, items at different prompt lengths; an
    item that has ended comes back unchanged and leaves the flag bits alone.  Tolerances: tests/test_gpu_lm_beam.py's step test's."""
    K, V, step, max_length, plen, ended, pen, ng, es, share, boost = STEP_CASES[case]
    B, ff = len(plen), 108
    rng = np.random.default_rng(400 + case)
    eos = V - 2
    state = LB.random_state(rng, B, K, V, step, max_length, ff, V - 1, plen, share)
    unsat = np.ones(B, np.int32)
    logits = rng.normal(0, 3, size=(B * K, V)).astype(np.float32)
    logits[:, :ff] += 4.0      # the banned range holds the largest logits
    if boost == "top":
        logits[:, eos] = logits.max(-1) + 2.0
    elif boost == "mid":
        logits[:, eos] = np.sort(logits[:, ff:], -1)[:, -2] - 0.01
    want = LB.beam_step(logits, K, step, max_length, eos, pen, ng, es, ff, plen, ended, *state, unsat)
    got = run_kernel_step(logits, K, step, max_length, eos, pen, ng, es, ff, plen, ended, state, unsat)
    for k in ("run_seq", "parent", "fin_seq", "fin_flag", "fin_len", "unsat", "ended"):
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    assert int(got["flags"][0]) == want["flags"]
    for k in ("run_score", "fin_score"):
        np.testing.assert_allclose(got[k], want[k], rtol=1e-5, atol=0)
    for b in np.nonzero(ended)[0]:      # unchanged, bit for bit
        rows = slice(b * K, (b + 1) * K)
        for k, a in zip(("run_seq", "run_score", "fin_seq", "fin_score", "fin_flag", "fin_len"), state):
            assert np.array_equal(got[k][rows], a[rows]), k
    # the frozen item alone: no flag bit at all
    only = [b for b in range(B) if ended[b]]
    sub = np.concatenate([np.arange(b * K, (b + 1) * K) for b in only])
    alone = run_kernel_step(logits[sub], K, step, max_length, eos, pen, ng, es, ff, [plen[b] for b in only], [1] * len(only), tuple(a[sub] for a in state),
                            unsat[only])
    assert int(alone["flags"][0]) == 0 and (alone["ended"] == 2).all()


# ---- 4. the beam attention against the plain attention on a cache gathered by the same table, bit for bit ----
def attn(q, kc, vc, tab, plen, K, heads, kv_heads, d, cap, tcap, step):
    from lds import native
    R = q.shape[0]
    out = torch.full_like(q, float("nan"))
    n = len(plen)
    native.check(native.lib().lds_test_llama_beam_attn(q.data_ptr(), kc.data_ptr(), vc.data_ptr(), tab.data_ptr() if tab is not None else None,
                                                       (C.c_int32 * n)(*[int(v) for v in plen]), R, K, heads, kv_heads, d, cap, tcap, step,
                                                       out.data_ptr(), native._stream()))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("shape", [(6, 2, 16), (4, 4, 192)])
@pytest.mark.parametrize("pos", [0, 1, 63, 64, 255, 256, 300])
def test_beam_attention_vs_plain_on_gathered_cache(shape, pos):
    heads, kv_heads, d = shape
    K, items, cap = 3, 2, 304
    R = items * K
    g = torch.Generator().manual_seed(pos * 7 + d)
    q = torch.randn(R, heads * d, generator=g).cuda()
    kc = torch.randn(R, kv_heads, cap, d, generator=g).cuda()
    vc = torch.randn(R, kv_heads, cap, d, generator=g).cuda()
    kc[:, :, pos + 1:], vc[:, :, pos + 1:] = float("nan"), float("nan")      # no key beyond the position is read
    for pl in sorted({min(p, pos + 1) for p in (1, 26, pos + 1)}):      # a prompt reaches at most up to the current position
        step = pos + 1 - pl
        tcap = max(step, 1)
        tab = torch.stack([torch.stack([torch.randperm(K, generator=g) + i * K for _ in range(tcap)], 1) for i in range(items)]).reshape(R, tcap)
        tab = tab.to(torch.int32).cuda()
        # the cache each beam row sees, gathered physically: prompt positions from the item's first row, generated ones by the table, the last its own
        src = torch.arange(R, device="cuda")[:, None].repeat(1, cap)
        src[:, :pl] = (torch.arange(R, device="cuda") // K * K)[:, None]
        if step > 1:
            src[:, pl:pos] = tab[:, :step - 1].long()
        gk = torch.gather(kc, 0, src[:, None, :, None].expand(R, kv_heads, cap, d)).contiguous()
        gv = torch.gather(vc, 0, src[:, None, :, None].expand(R, kv_heads, cap, d)).contiguous()
        got = attn(q, kc, vc, tab, [pl] * items, K, heads, kv_heads, d, cap, tcap, step)
        want = attn(q, gk, gv, None, [pl] * R, 1, heads, kv_heads, d, cap, 0, step)
        assert bool(torch.isfinite(want).all()) and torch.equal(got, want), (pl, step)
        # an identity table over per-row prompts of length 1 reproduces the plain kernel on the cache as it is
        if pl == 1:
            ident = torch.arange(R, dtype=torch.int32, device="cuda")[:, None].repeat(1, tcap).contiguous()
            assert torch.equal(attn(q, kc, vc, ident, [1] * R, 1, heads, kv_heads, d, cap, tcap, step), attn(q, kc, vc, None, [1] * R, 1, heads, kv_heads, d, cap, 0, step))


def test_beam_attention_at_the_longest_decode():
    """max_length 7488, the limit: the last step's 7488 keys take the most dynamic LDS any launch of the kernel asks for (a score and a source row
    per key: 65056 bytes, inside the 64 KiB a launch gets without further ado).  Bit for bit against the plain kernel on the gathered cache."""
    heads, kv_heads, d, K, cap, pl = 2, 1, 16, 2, 7488, 5
    pos = cap - 1
    step = pos + 1 - pl
    g = torch.Generator().manual_seed(11)
    q = torch.randn(K, heads * d, generator=g).cuda()
    kc = torch.randn(K, kv_heads, cap, d, generator=g).cuda()
    vc = torch.randn(K, kv_heads, cap, d, generator=g).cuda()
    tab = torch.randint(0, K, (K, step), generator=g).to(torch.int32).cuda()
    src = torch.arange(K, device="cuda")[:, None].repeat(1, cap)
    src[:, :pl] = 0
    src[:, pl:pos] = tab[:, :step - 1].long()
    gk = torch.gather(kc, 0, src[:, None, :, None].expand(K, kv_heads, cap, d)).contiguous()
    gv = torch.gather(vc, 0, src[:, None, :, None].expand(K, kv_heads, cap, d)).contiguous()
    got = attn(q, kc, vc, tab, [pl], K, heads, kv_heads, d, cap, step, step)
    want = attn(q, gk, gv, None, [pl] * K, 1, heads, kv_heads, d, cap, 0, step)
    assert bool(torch.isfinite(want).all()) and torch.equal(got, want)
    # one position more is refused
    from lds import native
    assert native.lib().lds_test_llama_beam_attn(q.data_ptr(), kc.data_ptr(), vc.data_ptr(), tab.data_ptr(), (C.c_int32 * 1)(pl), K, K, heads, kv_heads, d,
                                                 cap + 1, step, step, q.data_ptr(), native._stream()) == -1


# ---- 5. whole decodes against the restatement ----
def against_restatement(m, cfg, state, phones, max_length, K, es, margins_out=None):
    ids = LN.prompt_ids(cfg, phones)
    want, gap, steps = LB.generate_beam(state, cfg, m.inv_freq.numpy(), ids, K, max_length, early_stopping=ES[es])
    print(f"steps {steps}, smallest restatement margin {gap:.3e}")
    assert gap >= MIN_MARGIN      # margins first: every selection of the restatement's own run is clear of a tie
    ph = dev(np.asarray(phones, dtype=np.int64)[None])
    toks = m.generate(ph, ph, max_length=max_length, do_sample=False, num_beams=K, early_stopping=es).cpu().numpy()[0]
    assert np.array_equal(toks, want[len(ids):] - cfg["shift"]), (toks.tolist(), (want[len(ids):] - cfg["shift"]).tolist())
    return toks, steps


def test_reference_example_width_head_dim_192():
    """the width of the reference's own example (llama.py:186-193) with 2 layers: head_dim 192, kv_heads == heads, K = 2048 (vocab 2159: the
    36-values-per-lane step); four beams"""
    conf = dict(hidden_size=768, num_attention_heads=4, num_hidden_layers=2, intermediate_size=512, max_position_embeddings=256)
    m, cfg, state = build(conf, 2048, WIDE_SEED)
    assert cfg["head_dim"] == 192 and cfg["kv_heads"] == 4 and cfg["vocab"] == 2159
    against_restatement(m, cfg, state, (np.arange(15) * 7 % 107 + 1).astype(np.int64), 18 + 24, 4, True)


def test_toy_to_the_last_position(fx):
    """max_length == max_position_embeddings: the last table row, key counts across the 64-key blocks, ancestry over a hundred steps"""
    t = dict(fx["toy"])
    m, cfg, state = build(t, t.pop("semantic_kmeans_num"), LONG_SEED)
    toks, steps = against_restatement(m, cfg, state, fx["phone_r0"], cfg["max_pos"], 3, False)
    assert steps >= 80


# ---- 6. the workspace's contents, ids beyond the lengths and the poll interval change nothing; a repeat is bit-identical ----
def native_batch(m, fx, tag):
    phones = [fx["phone_r0"], fx["phone_r1"]]
    ph = np.full((2, 23), 77, dtype=np.int64)
    mask = np.zeros((2, 23), dtype=np.int64)
    for i, p in enumerate(phones):
        ph[i, :len(p)], mask[i, :len(p)] = p, 1
    return m.input_ids(dev(ph), dev(mask))


def test_nan_workspace_garbage_ids_and_repeat(fx):
    m, cfg, _ = case_model(fx, "beam4_penalty")
    nat = m.native()
    ids, lens = native_batch(m, fx, "beam4_penalty")
    args = dict(num_beams=4, repetition_penalty=1.3, no_repeat_ngram_size=2, early_stopping=True)
    t0 = nat.generate_beam(ids, lens, 48, **args)
    t1 = nat.generate_beam(ids, lens, 48, **args)
    assert torch.equal(t0, t1)
    assert nat.ws.bufs
    for buf in nat.ws.bufs.values():
        buf.fill_(255)      # every float a NaN, every table entry and flag -1
    bad = ids.clone()
    junk = torch.tensor([-7, 10 ** 12, 3], device="cuda").repeat(ids.shape[1])
    for b in range(2):
        bad[b, lens[b]:] = junk[: ids.shape[1] - lens[b]]
    t2 = nat.generate_beam(bad, lens, 48, **args)
    assert torch.equal(t0, t2)
    for b in range(2):      # and they are the recorded rows
        want = fx[f"beam4_penalty_r{b}_tokens"] + cfg["shift"]
        assert np.array_equal(t0[b, lens[b]:lens[b] + len(want)].cpu().numpy(), want)


def test_result_does_not_depend_on_the_poll_interval(fx):
    """the "eos" case's rows end after steps that are no multiples of one another's: whatever the interval, steps enqueued after an item's end
    change nothing"""
    from lds import native
    m, cfg, _ = case_model(fx, "eos")
    steps = [int(fx[f"eos_r{b}_steps"]) for b in range(2)]
    assert any(s % 8 for s in steps)
    nat = m.native()
    ids, lens = native_batch(m, fx, "eos")
    L = native.lib()
    B, P = ids.shape
    o = native.LMDecodeOpts(0, 0, 1.0, 1.0, 1.0, 0, 4, 0)
    nb = C.c_size_t()
    native.check(L.lds_llama_beam_workspace_bytes(nat.h, B, P, 48, 4, C.byref(nb)))
    pl = (C.c_int32 * B)(*[int(v) for v in lens])

    def polled(every):      # the decode through the test entry that takes the interval
        ws = torch.full((nb.value,), 255, dtype=torch.uint8, device="cuda")
        tokens = torch.empty(B, 48, dtype=torch.int64, device="cuda")
        n = C.c_int()
        native.check(L.lds_test_llama_generate_beam_poll(nat.h, ids.data_ptr(), C.cast(pl, C.c_void_p), B, P, 48, C.byref(o), tokens.data_ptr(), C.byref(n),
                                                         ws.data_ptr(), ws.numel(), native._stream(), every))
        return tokens[:, : n.value].contiguous()

    base = nat.generate_beam(ids, lens, 48, num_beams=4, early_stopping=False)
    for every in (1, 3, 7, 8, 64):
        assert torch.equal(polled(every), base), every
    assert L.lds_test_llama_generate_beam_poll(nat.h, ids.data_ptr(), C.cast(pl, C.c_void_p), B, P, 48, C.byref(o), None, None, None, 0, native._stream(), 0) == -1
    for b in range(2):
        want = fx[f"eos_r{b}_tokens"] + cfg["shift"]
        assert np.array_equal(base[b, lens[b]:lens[b] + len(want)].cpu().numpy(), want)


# ---- 7. every limit returns its code and enqueues nothing ----
def test_limits_return_codes_and_enqueue_nothing(fx):
    from lds import native
    m, cfg, _ = case_model(fx, "beam3")
    L = native.lib()
    nat = m.native()
    P, max_length = 9, 24
    nb = C.c_size_t()
    assert L.lds_llama_beam_workspace_bytes(nat.h, 2, P, max_length, 4, C.byref(nb)) == 0 and nb.value > 0
    need = nb.value
    err = L.lds_last_error

    def call(plen, B=2, ws_bytes=need, max_length=max_length, opts=None, entry="lds_llama_generate_beam"):
        o = opts or native.LMDecodeOpts(0, 5, 1.0, 1.0, 1.0, 0, 4, 1)
        ids = torch.zeros(B, P, dtype=torch.int64, device="cuda")
        tokens = torch.full((B, max_length), 7, dtype=torch.int64, device="cuda")
        ws = torch.zeros(ws_bytes, dtype=torch.uint8, device="cuda")
        n = C.c_int(-5)
        pl = (C.c_int32 * B)(*plen) if plen is not None else None
        plp = C.cast(pl, C.c_void_p) if pl else None
        if entry == "lds_llama_generate_beam":
            rc = L.lds_llama_generate_beam(nat.h, ids.data_ptr(), plp, B, P, max_length, C.byref(o), tokens.data_ptr(), C.byref(n), ws.data_ptr(), ws.numel(),
                                           native._stream())
        else:
            rc = L.lds_llama_generate(nat.h, ids.data_ptr(), plp, B, P, max_length, C.byref(o), None, tokens.data_ptr(), None, C.byref(n), ws.data_ptr(),
                                      ws.numel(), native._stream())
        torch.cuda.synchronize()
        assert bool((tokens == 7).all()) and n.value == -5 and not bool(ws.any()), "something ran"
        return rc

    O = native.LMDecodeOpts
    assert call([9, 9], opts=O(0, 5, 1.0, 1.0, 1.0, 0, 1, 1)) == -1 and b"num_beams" in err()
    assert call([9, 9], opts=O(0, 5, 1.0, 1.0, 1.0, 0, 9, 1)) == -1 and b"num_beams" in err()
    assert call([9, 9], opts=O(1, 5, 1.0, 1.0, 1.0, 0, 4, 1)) == -1 and b"beam sampling" in err()
    assert call([9, 9], opts=O(0, 5, 1.0, 1.0, 1.0, 0, 4, 3)) == -1 and b"early_stopping" in err()
    assert call([9, 9], opts=O(0, 5, 1.0, 1.0, 1.0, -1, 4, 1)) == -1 and b"no_repeat_ngram_size" in err()
    assert call([9] * 33, B=33, opts=O(0, 5, 1.0, 1.0, 1.0, 0, 8, 1)) == -1 and b"beam rows" in err()
    assert call([9] * 65, B=65, opts=O(0, 5, 1.0, 1.0, 1.0, 0, 2, 1)) == -1 and b"at most 64" in err()
    assert call([0, 9]) == -1 and b"in_len[0]" in err()
    assert call([9, 10]) == -1 and b"in_len[1]" in err()
    assert call([3, 9], max_length=9) == -1 and b"in_len[1]" in err() and b"max_length" in err()
    assert call(None, max_length=9) == -1 and b"max_length" in err()
    assert call([9, 9], max_length=cfg["max_pos"] + 1) == -1 and b"max_position_embeddings" in err()
    assert call([9, 9], max_length=7489) == -1 and b"max_length" in err()
    assert L.lds_llama_beam_workspace_bytes(nat.h, 33, P, max_length, 8, C.byref(nb)) == -1
    assert call([9, 9], ws_bytes=need - 256) == -2 and str(need).encode() in err()
    # the plain entry still refuses beams
    assert call([9, 9], opts=O(0, 5, 1.0, 1.0, 1.0, 0, 2, 1), entry="lds_llama_generate") == -1 and b"beam" in err()
    # a vocabulary above 4352 ids
    big, _, _ = build(dict(hidden_size=32, num_attention_heads=2, num_hidden_layers=1, intermediate_size=32, max_position_embeddings=32), 4242, 0)
    assert big.cfg["vocab"] == 4353
    with pytest.raises(NotImplementedError, match="4352"):
        big.generate(torch.ones(1, 3, dtype=torch.long).cuda(), None, do_sample=False, num_beams=2, max_length=16)
    ids = torch.zeros(1, P, dtype=torch.int64, device="cuda")
    tokens = torch.full((1, 24), 7, dtype=torch.int64, device="cuda")
    ws = torch.zeros(1 << 22, dtype=torch.uint8, device="cuda")
    n = C.c_int(-5)
    o = O(0, 5, 1.0, 1.0, 1.0, 0, 2, 1)
    assert L.lds_llama_generate_beam(big.native().h, ids.data_ptr(), None, 1, P, 24, C.byref(o), tokens.data_ptr(), C.byref(n), ws.data_ptr(), ws.numel(),
                                     native._stream()) == -1 and b"4352" in err()
    torch.cuda.synchronize()
    assert bool((tokens == 7).all()) and n.value == -5 and not bool(ws.any())
