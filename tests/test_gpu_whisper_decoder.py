"""Whisper's text decoder on the GPU (include/lds.h lds_whisper_decoder_*, encoder.whisper.model.Whisper(dims, decoder=True)): the
teacher-forced logits and the greedy decode against the fixtures recorded from the reference's blocks in float64
(tests/golden/make_whisper_decoder_fixtures.py), the two entry points against each other bit for bit, the ragged-batch invariants, the
vocabulary head alone at large-v3's 51,866 columns against the float64 restatement (tests/whisper_decoder_numpy.py), and the refusals."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import whisper_decoder_numpy as dnp
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

TOL = 2e-5              # x absmax: the project's bound for an fp32 forward against the reference (tests/test_gpu_units.py)
_CACHE = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def fixtures():
    if "z" not in _CACHE:
        _CACHE["z"] = dict(np.load(os.path.join(GOLDEN, "whisper_decoder.npz")))
    return _CACHE["z"]


def setup(name):
    """(the native decoder, the seeded inputs, the state) of configuration `name` at the fixture's seed; built once"""
    from lds import arch, init_weights, native
    if name not in _CACHE:
        c, seed = dnp.CONFIGS[name], int(fixtures()[f"seed_{name}"])
        state = arch.whisper_decoder_init_state(c["n_vocab"], c["n_text_ctx"], c["n_state"], c["n_layer"], seed)
        dec = native.WhisperDecoder(c["n_vocab"], c["n_text_ctx"], c["n_state"], c["n_head"], c["n_layer"], 1500, state)
        _CACHE[name] = (dec, dnp.inputs(name, init_weights.uniform, seed), state)
    return _CACHE[name]


def prompt_tensor(prompts, fill):
    return dev(dnp.pad_rows(prompts, max(len(p) for p in prompts), int(fill))), [len(p) for p in prompts]


def generate(name, rows=(0, 1, 2), units=None, n_frames=None, return_logits=False, **kw):
    dec, inp, _ = setup(name)
    c = dnp.CONFIGS[name]
    rows = list(rows)
    u = dev(inp["units"][rows]) if units is None else units
    dec.cross(u, [dnp.N_FRAMES[b] for b in rows] if n_frames is None else n_frames)
    ids, plen = prompt_tensor([inp["prompts"][b] for b in rows], inp["eos"])
    kw.setdefault("suppress", inp["suppress"])
    kw.setdefault("begin_suppress", inp["begin_suppress"])
    return dec.generate(ids, plen, c["max_new"], inp["eos"], inp["eos"], return_logits=return_logits, **kw), plen


@pytest.mark.parametrize("name", ["A", "B", "C", "A1500"])
def test_logits_vs_reference(name, record_margin):
    """lds_whisper_decoder_logits on the ragged batch (n_frames 1, 37, 100; tok_len 9, 5, 2) against the float64 oracle"""
    z = fixtures()
    cfgname = name[0]
    dec, inp, _ = setup(cfgname)
    if name == "A1500":
        dec.cross(dev(inp["units_long"]))
        got = dec.logits(dev(inp["tf_tokens"][:1]))
    else:
        dec.cross(dev(inp["units"]), dnp.N_FRAMES)
        got = dec.logits(dev(inp["tf_tokens"]), dev(np.array(dnp.TF_LEN, dtype=np.int32)))
    ref = z[f"logits_{name}"]
    assert tuple(got.shape) == ref.shape
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max() / np.abs(ref).max())
    print(f"decoder logits {name}: {err:.3e} x absmax ({err / float(z[f'gap_{name}']):.2f} x the oracle's own fp32-vs-fp64 gap {float(z[f'gap_{name}']):.2e})")
    record_margin(err, TOL)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_generate_vs_reference(name, record_margin):
    """greedy ids equal the oracle's exactly (its paths keep a top-2 gap of margin_X >= 1e-3 x absmax, 50 x the logits bound); the chosen
    ids' log-probs within TOL x absmax(logits); A runs into n_text_ctx = 32: every row stops there, not at max_new_tokens = 40"""
    z = fixtures()
    assert float(z[f"margin_{name}"]) >= 1e-3
    (toks, tlp, slp, _), plen = generate(name)
    ref_t, ref_len, ref_lp = z[f"gen_tokens_{name}"], z[f"gen_len_{name}"], z[f"gen_lp_{name}"]
    assert toks.cpu().numpy().tolist() == ref_t.tolist()
    if name == "A":
        assert ref_len.tolist() == [32, 32, 32] and toks.shape[1] == 32
    got_lp = tlp.cpu().numpy().astype(np.float64)
    assert got_lp.shape == ref_lp.shape
    err = float(np.abs(got_lp - ref_lp).max() / float(z[f"gen_absmax_{name}"]))
    print(f"decoder generate {name}: ids identical over {[int(n) - p for n, p in zip(ref_len, plen)]} steps, log-prob error {err:.3e} x absmax")
    record_margin(err, TOL)
    # sum_logprob: the fp32 sum of the row's log-probs in step order
    want = np.zeros(3, dtype=np.float32)
    for i in range(tlp.shape[1]):
        want += tlp[:, i].cpu().numpy()
    assert np.array_equal(slp.cpu().numpy(), want)


def test_generate_long_audio(record_margin):
    """one row over 1500 cross keys (A)"""
    z = fixtures()
    dec, inp, _ = setup("A")
    (toks, tlp, _, _), _ = generate("A", rows=[2], units=dev(inp["units_long"]), n_frames=[dnp.T_LONG])
    assert toks.cpu().numpy().tolist() == z["gen_tokens_A1500"].tolist()
    record_margin(float(np.abs(tlp.cpu().numpy() - z["gen_lp_A1500"]).max() / float(z["gen_absmax_A1500"])), TOL)


@pytest.mark.parametrize("name", ["A", "B"])
def test_generate_logits_equal_logits_entry(name):
    """prefill rows and decode steps go through the same kernels: generate's logits_out equals lds_whisper_decoder_logits on the produced
    sequence BIT FOR BIT (row b's step s is position prompt_len[b] - 1 + s)"""
    dec, inp, _ = setup(name)
    (toks, _, _, lg), plen = generate(name, return_logits=True)
    z = fixtures()
    full = dec.logits(toks)
    for b in range(3):
        for s in range(int(z[f"gen_len_{name}"][b]) - plen[b]):
            assert torch.equal(lg[s, b], full[b, plen[b] - 1 + s]), (b, s)


def test_rows_alone_repeat_and_poison():
    """every row of the ragged batch equals its B = 1 run bit for bit (tokens, log-probs, logits); a repeat gives identical bits; NaN
    beyond n_frames[b] in units and a NaN-filled workspace change nothing"""
    dec, inp, _ = setup("B")
    (t0, lp0, s0, lg0), plen = generate("B", return_logits=True)
    dec.cross(dev(inp["units"]), dnp.N_FRAMES)
    tf, tl = dev(inp["tf_tokens"]), dev(np.array(dnp.TF_LEN, dtype=np.int32))
    full0 = dec.logits(tf, tl)
    # repeat, with poison: NaN behind every clip's frames, the workspace filled with 0xFF bytes (NaN) before `cross`
    units = inp["units"].copy()
    for b, n in enumerate(dnp.N_FRAMES):
        units[b, n:] = np.nan
    for buf in dec.ws.bufs.values():
        buf.fill_(255)
    (t1, lp1, s1, lg1), _ = generate("B", units=dev(units), return_logits=True)
    assert torch.equal(t0, t1) and torch.equal(lp0, lp1) and torch.equal(s0, s1) and torch.equal(lg0, lg1)
    assert torch.equal(dec.logits(tf, tl), full0)
    z = fixtures()
    for b in range(3):
        (tb, lpb, sb, lgb), _ = generate("B", rows=[b], units=dev(units[b:b + 1, : dnp.N_FRAMES[b]].copy()), n_frames=[dnp.N_FRAMES[b]], return_logits=True)
        n = int(z["gen_len_B"][b])
        assert tb[0].tolist() == t0[b, :n].tolist() and torch.equal(lpb[0], lp0[b]) and torch.equal(sb[0], s0[b])
        assert torch.equal(lgb[: n - plen[b], 0], lg0[: n - plen[b], b])
        assert torch.equal(dec.logits(tf[b:b + 1], tl[b:b + 1])[0], full0[b])


def test_eos_forced_and_begin_suppress():
    """everything but EOS suppressed: every row emits EOS at once with log-prob 0 and stops.  begin_suppress acts on each row's first
    generated step only: banning a row's first id changes that step (to the restatement's choice under the ban); banning an id that the
    path takes at a LATER step changes nothing."""
    dec, inp, _ = setup("B")
    c, eos = dnp.CONFIGS["B"], inp["eos"]
    (toks, tlp, slp, _), plen = generate("B", suppress=[i for i in range(c["n_vocab"]) if i != eos], begin_suppress=None)
    assert toks.shape[1] == max(plen) + 1
    for b in range(3):
        assert toks[b, plen[b]].item() == eos and toks[b, plen[b] + 1:].eq(eos).all()
    assert tlp[:, 0].eq(0).all() and tlp[:, 1:].eq(0).all() and slp.eq(0).all()
    (base, _, _, lg), _ = generate("B", return_logits=True)
    base = base.cpu().numpy()
    b = 2
    gen = base[b, plen[b]:].tolist()
    later = next(t for t in gen[1:] if t != gen[0])      # (the fixture's path: distinct ids along it)
    (same, _, _, _), _ = generate("B", begin_suppress=list(inp["begin_suppress"]) + [later])
    assert same.cpu().numpy().tolist() == base.tolist()
    (other, _, _, _), _ = generate("B", begin_suppress=list(inp["begin_suppress"]) + [gen[0]])
    want, _, _ = dnp.choose(lg[0, b].cpu().numpy(), list(inp["suppress"]) + list(inp["begin_suppress"]) + [gen[0]])
    assert other[b, plen[b]].item() == want != gen[0]


@pytest.mark.parametrize("n_suppress", [0, 1, 90])
def test_head_alone_large_vocab(n_suppress, record_margin):
    """the head at n_vocab = 51866 (1621 tiles, the last of 26 columns), n_state = 128, 3 rows, through lds_test_whisper_head: token,
    log-prob and log-sum-exp against float64.  Row 0: its winner planted in the last partial tile.  Row 1: two identical embedding rows
    (ids 1000 and 40000) planted as joint winners -- an exact tie, which must give the lower id.  Row 2: seeded.  Suppress lists of 0, 1 and
    90 ids, which take out row 2's unsuppressed winner (and the runners-up)."""
    from lds import init_weights as iw, native
    V, K = 51866, 128
    x = iw.uniform("wdec.head.x", (3, K), 0, -2, 2)
    E = iw.uniform("wdec.head.E", (V, K), 0, -1, 1).copy()
    g, bt = iw.uniform("wdec.head.g", (K,), 0, 0.8, 1.2), iw.uniform("wdec.head.b", (K,), 0, -0.1, 0.1)
    xn = dnp.layer_norm(x.astype(np.float64), g.astype(np.float64), bt.astype(np.float64))
    E[V - 3] = (xn[0] / np.abs(xn[0]).max()).astype(np.float32)
    E[1000] = E[40000] = (xn[1] / np.abs(xn[1]).max()).astype(np.float32)
    ref = xn @ E.astype(np.float64).T
    assert int(ref[0].argmax()) == V - 3 and sorted(np.argsort(ref[1])[-2:].tolist()) == [1000, 40000]
    order = [i for i in np.argsort(-ref[2]).tolist() if i not in (V - 3, 1000, 40000)]
    sup = sorted(order[:n_suppress])
    tok, lp, lse, lg = native.whisper_head_test(dev(x), dev(g), dev(bt), dev(np.ascontiguousarray(E.T)), sup, return_logits=True)
    absmax = float(np.abs(ref).max())
    err = float(np.abs(lg.cpu().numpy() - ref).max() / absmax)
    for r in range(3):
        want_tok, want_lp, want_lse = dnp.choose(ref[r], sup)
        if r == 1:
            want_tok = 1000
        else:
            assert dnp.top2_gap(ref[r], sup) > 10 * TOL * absmax      # (two logits, each within TOL x absmax, cannot swap)
        assert tok[r].item() == want_tok, (r, tok[r].item(), want_tok)
        err = max(err, abs(lp[r].item() - (want_lp if r != 1 else dnp.choose(ref[r], sup)[1])) / absmax, abs(lse[r].item() - want_lse) / absmax)
    print(f"head alone, {n_suppress} suppressed: tokens {tok.tolist()}, worst error {err:.3e} x absmax")
    record_margin(err, TOL)


def test_python_model_matches_handle():
    """encoder.whisper.model.Whisper(dims, decoder=True): load_state_dict of decoder.* keys, logits / decode / score / detect_language"""
    from encoder.whisper.model import ModelDimensions, Whisper
    dec, inp, state = setup("B")
    c = dnp.CONFIGS["B"]
    m = Whisper(ModelDimensions(80, 1500, 64, 1, 1, c["n_vocab"], c["n_text_ctx"], c["n_state"], c["n_head"], c["n_layer"]), decoder=True)
    missing, unexpected = m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=False)
    assert not unexpected and all(k.startswith("encoder.") for k in missing)
    units = dev(inp["units"])
    dec.cross(units, dnp.N_FRAMES)
    tf = dev(inp["tf_tokens"])
    want = dec.logits(tf)
    assert torch.equal(m.decoder(tf, units, dnp.N_FRAMES), want)
    (t0, lp0, s0, _), plen = generate("B")
    toks, tlp, avg = m.decode(units, dnp.N_FRAMES, prompt=inp["prompts"], max_new_tokens=c["max_new"], suppress_tokens=inp["suppress"],
                              begin_suppress_tokens=inp["begin_suppress"], eot=inp["eos"])
    assert torch.equal(toks, t0) and torch.equal(tlp, lp0)
    n_gen = torch.as_tensor([int(n) - p for n, p in zip(fixtures()["gen_len_B"], plen)], device="cuda", dtype=torch.float32)
    assert torch.equal(avg, s0 / n_gen)
    lp, ranks, loss, n, _ = m.score(units, tf, dnp.TF_LEN, dnp.N_FRAMES)
    ref = torch.log_softmax(dec.logits(tf, dev(np.array(dnp.TF_LEN, dtype=np.int32))).double(), -1)
    for b, L in enumerate(dnp.TF_LEN):
        for t in range(L - 1):
            assert abs(lp[b, t].item() - ref[b, t, tf[b, t + 1]].item()) < 1e-4
        assert lp[b, L - 1:].eq(0).all() and ranks[b, L - 1:].eq(-1).all()
    assert n.item() == sum(L - 1 for L in dnp.TF_LEN)
    with pytest.raises(NotImplementedError):
        m.decode(units, temperature=0.2)
    with pytest.raises(NotImplementedError):
        m.decode(units, beam_size=5)


def test_refusals():
    """S > n_text_ctx, n_frames > T, a small workspace (LDS_ENOMEM with the size), a missing tensor (LDS_EMISSING with the name), the
    out-of-scope options -- all before anything is enqueued"""
    from lds import native
    dec, inp, state = setup("A")
    L = native.lib()
    units = dev(inp["units"])
    dec.cross(units, dnp.N_FRAMES)
    with pytest.raises(RuntimeError, match="n_text_ctx"):
        dec.logits(dev(np.zeros((3, 33), dtype=np.int64)))
    ws = torch.empty(dec.workspace_bytes(3, dnp.T_PAD, 9), dtype=torch.uint8, device="cuda")
    nf = np.array([1, 37, dnp.T_PAD + 1], dtype=np.int32)
    rc = L.lds_whisper_decoder_cross(dec.h, units.data_ptr(), nf.ctypes.data, 3, dnp.T_PAD, ws.data_ptr(), ws.numel(), None)
    assert rc != 0 and "n_frames[2] = 101" in L.lds_last_error().decode()
    rc = L.lds_whisper_decoder_cross(dec.h, units.data_ptr(), None, 3, dnp.T_PAD, ws.data_ptr(), 4096, None)
    need = dec.workspace_bytes(3, dnp.T_PAD, 2)
    assert rc != 0 and f"need {need} bytes" in L.lds_last_error().decode()
    short = {k: v for k, v in state.items() if k != "decoder.blocks.1.cross_attn.key.weight"}
    c = dnp.CONFIGS["A"]
    with pytest.raises(RuntimeError, match=r"decoder\.blocks\.1\.cross_attn\.key\.weight \(absent\)"):
        native.WhisperDecoder(c["n_vocab"], c["n_text_ctx"], c["n_state"], c["n_head"], c["n_layer"], 1500, short)
    ids, plen = prompt_tensor(inp["prompts"], inp["eos"])
    for kw, msg in ((dict(no_repeat_ngram_size=3), "no_repeat_ngram_size"), (dict(num_beams=4), "beam search"), (dict(temperature=0.5), "temperature"),
                    (dict(cap=33), "n_text_ctx")):
        with pytest.raises(RuntimeError, match=msg):
            dec.generate(ids, plen, 4, inp["eos"], inp["eos"], **kw)
