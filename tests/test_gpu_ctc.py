"""CTC heads on a real MI355X (csrc/ctc.hip through lds.native and encoder.ctc.CTCHead): head statistics against float64 under the
a-priori bounds of tests/ctc_numpy.py, bit-for-bit invariances, the forward and Viterbi recursions on given emissions, the greedy
collapse, the public score / align, audio -> native encoder -> head against transformers' *ForCTC (tests/golden/ctc.npz) and the tool."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ctc_numpy as CN
from conftest import ROOT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

L_LADDER = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 510, 511)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_head(N, V, D, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((N, D)) * scale).astype(np.float32)
    W = (rng.standard_normal((V, D)) / np.sqrt(D)).astype(np.float32)
    b = (rng.standard_normal(V) * 0.5).astype(np.float32)
    return X, W, b


def run_head(X, W, b, n_frames=None, logprobs=False, ws=None):
    """X [N, D] (one clip) or [B, T, D] -> numpy (arg, m, lse[, log-probs])"""
    from lds import native
    if X.ndim == 2:
        X, n_frames = X[None], [X.shape[0]]
    out = native.ctc_head(dev(X), n_frames, dev(W), dev(b), return_logprobs=logprobs, ws=ws)
    return tuple(o.cpu().numpy() for o in out)


def head_fractions(X, W, b, arg, m, lse):
    """(worst |m - z64[arg]| / delta_z, worst |lse - lse64| / delta_lse, worst arg criterion / (2 delta_z), ids differing outside the gap)"""
    z, a64, _, l64 = CN.head_stats(X, W, b)
    dz = CN.delta_z(X, W, b)
    rows = np.arange(len(X))
    assert ((arg >= 0) & (arg < len(W))).all()
    fm = float((np.abs(m - z[rows, arg]) / dz[rows, arg]).max())
    fl = float((np.abs(lse - l64) / CN.delta_lse(X, W, b, l64)).max())
    fa = float(((z[rows, a64] - z[rows, arg]) / (dz[rows, a64] + dz[rows, arg])).max())
    clear = CN.top2_gap(z) > 2 * dz.max(axis=1)
    return fm, fl, fa, int((arg[clear] != a64[clear]).sum())


def test_head_statistics_against_float64(record_margin):
    """(arg, m, lse) under bounds 1 and 2 on every shape class: one column, odd sizes below a tile, several column splits with a 3-column
    tail tile, many row blocks; logits of magnitude 3e4; arg equal to float64's wherever the float64 gap exceeds 2 delta_z"""
    worst = 0.0
    for N, V, D, scale in ((1, 2, 8, 1.0), (333, 33, 136, 1.0), (70, 4099, 1024, 1.0), (70000, 32, 64, 1.0), (40, 33, 136, 1e4)):
        X, W, b = make_head(N, V, D, seed=N + V, scale=scale)
        arg, m, lse = run_head(X, W, b)
        assert np.isfinite(lse).all() and np.isfinite(m).all()
        fm, fl, fa, wrong = head_fractions(X, W, b, arg[0], m[0], lse[0])
        print(f"head N={N} V={V} D={D} scale={scale:g}: m {fm:.3g} of bound 1, lse {fl:.3g} of bound 2, arg criterion {fa:.3g}, ids differing outside the gap {wrong}; "
              f"max |z| {np.abs(m).max():.3g}")
        assert wrong == 0
        worst = max(worst, fm, fl, fa)
    record_margin(worst, 1.0)


def test_head_planted_maxima_and_ties():
    """a row whose maximum sits in the first column tile, one where it sits in the last (a 3-column tail tile of another split); two
    identical columns inside a tile and in different splits: the lowest id"""
    X, W, b = make_head(8, 4099, 136, seed=3)
    W[20], b[20] = W[7], b[7]              # the same tile
    W[4098], b[4098] = W[100], b[100]      # the first split and the last
    W[4097], b[4097] = W[4096], b[4096]    # inside the tail tile
    for r, v in enumerate((3, 4095, 7, 20, 100, 4098, 4096, 4097)):
        X[r] = 30.0 * W[v] / float(W[v] @ W[v])
    arg, m, lse = run_head(X, W, b)
    assert arg[0].tolist() == [3, 4095, 7, 7, 100, 100, 4096, 4096]
    z = CN.head_stats(X, W, b)[0]
    assert np.array_equal(arg[0], z.argmax(axis=1))


def test_head_ragged_and_logprobs(record_margin):
    """a ragged [3][50] batch with lengths (50, 1, 0) and NaN beyond them: valid frames under the bounds, padded frames arg -1 / m 0 / lse 0,
    logprobs_out = z - lse within delta_z + delta_lse and zeros in padded rows"""
    B, T, V, D = 3, 50, 33, 136
    X, W, b = make_head(B * T, V, D, seed=11)
    lens = np.array([50, 1, 0])
    valid = (np.arange(T)[None, :] < lens[:, None]).reshape(-1)
    Xp = X.copy()
    Xp[~valid] = np.nan
    arg, m, lse, lp = run_head(Xp.reshape(B, T, D), W, b, n_frames=lens, logprobs=True)
    arg, m, lse, lp = arg.reshape(-1), m.reshape(-1), lse.reshape(-1), lp.reshape(-1, V)
    assert (arg[~valid] == -1).all() and (m[~valid] == 0).all() and (lse[~valid] == 0).all() and (lp[~valid] == 0).all()
    Xv = X[valid]
    fm, fl, fa, wrong = head_fractions(Xv, W, b, arg[valid], m[valid], lse[valid])
    z, _, _, l64 = CN.head_stats(Xv, W, b)
    tol = CN.delta_z(Xv, W, b) + CN.delta_lse(Xv, W, b, l64)[:, None]
    fp = float((np.abs(lp[valid] - (z - l64[:, None])) / tol).max())
    print(f"ragged head: m {fm:.3g}, lse {fl:.3g}, arg {fa:.3g}, log-probs {fp:.3g} of their bounds")
    assert wrong == 0
    record_margin(max(fm, fl, fa, fp), 1.0)
    # the dense and ragged forms agree bit for bit on the valid rows
    a2, m2, l2 = run_head(Xv, W, b)
    assert np.array_equal(a2[0], arg[valid]) and np.array_equal(m2[0], m[valid]) and np.array_equal(l2[0], lse[valid])


def test_head_invariances_bit_for_bit():
    """repeats; a frame alone and inside N = 3, 1500, 12,000 at other positions; NaN / Inf in other rows; a poisoned workspace"""
    from lds import native
    V, D = 4099, 136
    X, W, b = make_head(12000, V, D, seed=5)
    frame = X[777].copy()
    base = run_head(frame[None], W, b, logprobs=True)
    assert np.isfinite(base[2]).all()
    for N, at in ((3, 1), (1500, 1499), (12000, 129)):
        Xn = X[:N].copy()
        Xn[at] = frame
        for poison in (None, np.nan, np.inf):
            if poison is not None:
                Xn[np.arange(N) != at] = poison
            got = run_head(Xn, W, b, logprobs=N <= 1500)
            for g, r in zip(got, base):
                assert np.array_equal(g[0, at], r[0, 0]), (N, at, poison)
    Xn = X[:1500]
    nb = native._bytes("lds_ctc_head_workspace_bytes", 1, 1500, V, D)
    outs = []
    for pattern in (0, 0x7fc07fc0, 0x7fc07fc0):
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        native.debug_fill(ws, pattern)
        outs.append(run_head(Xn, W, b, logprobs=True, ws=ws))
    for o in outs[1:]:
        for g, r in zip(o, outs[0]):
            assert np.array_equal(g, r)


# ---- the recursions on given emissions ----
def rand_emissions(rng, T, L, V=32):
    """fp32 emissions [T, L + 1] cut out of a random log-softmax over V symbols, and labels in 1 .. V - 1"""
    z = rng.standard_normal((T, V))
    lp = z - np.log(np.exp(z).sum(axis=1, keepdims=True))
    labels = rng.integers(1, V, L)
    return CN.emissions(lp, labels, 0).astype(np.float32), labels


def run_trellis(cases):
    """cases: [(E [T, L + 1] fp32, labels [L], n_frames)] -> per case (nll, path_score, frame_label [T], segments [L, 2], label_logprob [L]);
    one ragged batch, everything beyond a clip's frames and labels NaN"""
    from lds import native
    B = len(cases)
    T = max(max(E.shape[0] for E, _, _ in cases), 1)
    Lmax = max(max(len(l) for _, l, _ in cases), 1)
    Eb = np.full((B, T, Lmax + 1), np.nan, dtype=np.float32)
    lab = np.zeros((B, Lmax), dtype=np.int64)
    for i, (E, l, n) in enumerate(cases):
        Eb[i, :n, :len(l) + 1] = E[:n, :len(l) + 1]
        lab[i, :len(l)] = l
    nf, ll = [n for _, _, n in cases], [len(l) for _, l, _ in cases]
    Ed, labd = dev(Eb), dev(lab)
    nll = native.ctc_test_forward(Ed, nf, labd, ll).cpu().numpy()
    ps, fl, seg, llp = (t.cpu().numpy() for t in native.ctc_test_viterbi(Ed, nf, labd, ll))
    return [(float(nll[i]), float(ps[i]), fl[i], seg[i, :ll[i]], llp[i, :ll[i]], seg[i, ll[i]:]) for i in range(B)]


def check_case(E, labels, n, got):
    """-> (forward fraction of bound 3, Viterbi fraction of bound 3); asserts the structural properties"""
    nll, ps, fl, seg, llp, seg_rest = got
    L = len(labels)
    E = E[:n, :L + 1]
    ref, A = CN.forward(E, labels)
    opt = CN.viterbi(E, labels)[0]
    assert (seg_rest == -1).all() and (fl[n:] == -1).all()
    if not np.isfinite(ref):
        assert nll == np.inf and ps == -np.inf and (seg == -1).all() and (fl == -1).all() and (llp == 0).all()
        return 0.0, 0.0
    bound = CN.bound3(max(n, 1), A)
    f_fwd = abs(nll - ref) / bound
    path = fl[:n]
    assert CN.path_states_valid(path, L) and CN.path_respects_repeats(path, labels)
    mine = CN.path_score(E, path) if n else 0.0
    f_vit = max(abs(mine - opt), abs(ps - opt)) / bound
    for l in range(L):      # segments and label_logprob restate frame_label
        at = np.nonzero(path == l)[0]
        assert len(at) and seg[l, 0] == at[0] and seg[l, 1] == at[-1] + 1 and len(at) == seg[l, 1] - seg[l, 0]
        mean = E[at, l + 1].astype(np.float64).mean()
        assert abs(llp[l] - mean) <= 2 * CN.U * max(abs(mean), 1e-30)
    return f_fwd, f_vit


def test_trellis_small_and_single_path_cases(record_margin):
    """L = 0; T = 1, L = 1; T = L without repeats and T = L + r with r adjacent repeats (a single path: nll = -sum E[t][l_t], the alignment is
    forced); one frame fewer (+inf, (-1, -1) segments); labels [a, a, b]; no frames at all; a ragged batch with NaN beyond lengths"""
    rng = np.random.default_rng(21)
    cases = []
    E, _ = rand_emissions(rng, 9, 0)
    cases.append((E, np.zeros(0, dtype=np.int64), 9))                                  # 0: L = 0
    E, l = rand_emissions(rng, 1, 1)
    cases.append((E, l, 1))                                                            # 1: T = 1, L = 1
    E, _ = rand_emissions(rng, 20, 20)
    diag = 1 + np.arange(20) % 31
    cases.append((E, diag, 20))                                                        # 2: T = L, no repeats: the diagonal
    rep = np.array([5, 5, 6, 7, 7, 7, 8, 9, 9, 3])                                      # 4 adjacent repeats
    E, _ = rand_emissions(rng, 14, 10)
    cases.append((E, rep, 14))                                                         # 3: T = L + r: a single path
    cases.append((E, rep, 13))                                                         # 4: one frame fewer: infeasible
    E, _ = rand_emissions(rng, 7, 3)
    cases.append((E, np.array([4, 4, 9]), 7))                                          # 5: [a, a, b]
    cases.append((E, np.array([4, 4, 9]), 0))                                          # 6: no frames, L > 0: +inf
    cases.append((E, np.zeros(0, dtype=np.int64), 0))                                  # 7: no frames, L = 0: 0
    got = run_trellis(cases)
    fr = [check_case(E, l, n, g) for (E, l, n), g in zip(cases, got)]
    # the forced alignments
    assert got[0][0] == pytest.approx(-float(cases[0][0][:, 0].astype(np.float64).sum()), rel=1e-6)
    assert got[2][2][:20].tolist() == list(range(20))
    assert got[2][0] == pytest.approx(-sum(float(cases[2][0][t, t + 1]) for t in range(20)), rel=1e-6)
    assert got[3][2][:14].tolist() == [0, -1, 1, 2, 3, -1, 4, -1, 5, 6, 7, -1, 8, 9]
    assert got[4][0] == np.inf and got[6][0] == np.inf and got[6][1] == -np.inf
    assert got[7][0] == 0.0 and got[7][1] == 0.0
    print("small trellis cases, fractions of bound 3 (forward, Viterbi):", [(round(a, 4), round(b, 4)) for a, b in fr])
    record_margin(max(max(a, b) for a, b in fr), 1.0)


def test_trellis_label_ladder(record_margin):
    """L at every lane and dword boundary of the one-wave layout (16 states per lane, 64 lanes) with T = L + 40: one loop, its worst"""
    rng = np.random.default_rng(22)
    cases = []
    for L in L_LADDER:
        E, l = rand_emissions(rng, L + 40, L)
        assert CN.feasible(L + 40, l)
        cases.append((E, l, L + 40))
    got = run_trellis(cases)
    fr = [check_case(E, l, n, g) for (E, l, n), g in zip(cases, got)]
    print("ladder, fractions of bound 3 (forward, Viterbi):", {L: (round(a, 4), round(b, 4)) for L, (a, b) in zip(L_LADDER, fr)})
    record_margin(max(max(a, b) for a, b in fr), 1.0)


def test_trellis_long_scaled_and_planted(record_margin):
    """T = 1499, L = 300 with repeats; the same emissions scaled by 20 (alpha beyond -1e5); a planted alignment (the intended path at -0.01
    per frame, everything else <= -5) must come back exactly"""
    rng = np.random.default_rng(23)
    T, L = 1499, 300
    E, l = rand_emissions(rng, T, L)
    l[10::10] = l[9::10][:len(l[10::10])]      # every tenth label repeats the one before
    assert CN.feasible(T, l) and sum(a == b for a, b in zip(l, l[1:])) >= 29
    E20 = (E * 20).astype(np.float32)
    # planted: label k holds frames [3 k + 1, 3 k + 3), a blank between
    Lp, Tp = 100, 320
    lp = rng.integers(1, 32, Lp)
    lp[1::7] = lp[0::7][:len(lp[1::7])]
    Ep = (-5.0 - rng.random((Tp, Lp + 1)) * 3).astype(np.float32)
    want = np.full(Tp, -1)
    for k in range(Lp):
        want[3 * k + 1:3 * k + 3] = k
    for t in range(Tp):
        Ep[t, 0 if want[t] < 0 else want[t] + 1] = -0.01
    cases = [(E, l, T), (E20, l, T), (Ep, lp, Tp)]
    got = run_trellis(cases)
    fr = [check_case(Ec, lc, n, g) for (Ec, lc, n), g in zip(cases, got)]
    assert abs(CN.forward(E20, l)[1]) > 1e5
    assert np.array_equal(got[2][2][:Tp], want)
    assert got[2][3].tolist() == [[3 * k + 1, 3 * k + 3] for k in range(Lp)]
    print("long / scaled / planted, fractions of bound 3 (forward, Viterbi):", [(round(a, 4), round(b, 4)) for a, b in fr])
    record_margin(max(max(a, b) for a, b in fr), 1.0)


# ---- greedy ----
def test_greedy_planted_strings_are_integer_exact():
    """all blank, a leading repeat, a a _ a, a token on the last frame, T = 1, length 0, a run across the pieces of the workgroup's threads"""
    from lds import native
    rng = np.random.default_rng(31)
    strings = [[0, 0, 0, 0], [3, 3, 0, 5], [4, 4, 0, 4], [0, 0, 0, 9], [7], [], [0] * 5 + [2] * 600 + [0, 2, 2, 3] + [1] * 300,
               rng.integers(0, 4, 1000).tolist()]
    B, T = len(strings), max(len(s) for s in strings)
    arg = np.full((B, T), 17, dtype=np.int32)
    for i, s in enumerate(strings):
        arg[i, :len(s)] = s
    m = rng.standard_normal((B, T)).astype(np.float32)
    lse = (m + rng.random((B, T)).astype(np.float32) * 3).astype(np.float32)
    nf = [len(s) for s in strings]
    tok, n, start, length, lp = (t.cpu().numpy() for t in native.ctc_greedy(dev(arg), dev(m), dev(lse), nf, 0, pad_id=-9))
    for i, s in enumerate(strings):
        d32 = (m[i, :len(s)] - lse[i, :len(s)]).astype(np.float32)      # the kernel's fp32 difference, then a double mean
        want = CN.greedy(s, d32, np.zeros_like(d32), 0)
        k = len(want[0])
        assert n[i] == k
        assert np.array_equal(tok[i, :k], want[0]) and np.array_equal(start[i, :k], want[1]) and np.array_equal(length[i, :k], want[2])
        assert (np.abs(lp[i, :k] - want[3]) <= 2 * CN.U * np.abs(want[3])).all()      # (a double sum in frame order, rounded once)
        assert (tok[i, k:] == -9).all() and (start[i, k:] == -1).all() and (length[i, k:] == 0).all() and (lp[i, k:] == 0).all()


def test_greedy_on_a_head_run(record_margin):
    """head + collapse against ctc_numpy on the device's own ids (integer-exact) and, where no frame sits inside the gap, on float64's;
    logprob under bound 2 (+ bound 1 for m)"""
    from encoder.ctc import CTCHead
    B, T, V, D = 2, 200, 33, 136
    X, W, b = make_head(B * T, V, D, seed=41)
    b[0] += 3.0      # blanks often win: runs and gaps
    head = CTCHead(W, b, blank=0)
    lens = [200, 123]
    out = head.greedy(dev(X.reshape(B, T, D)), lens)
    worst = 0.0
    for i in range(B):
        Xi = X.reshape(B, T, D)[i, :lens[i]]
        z, a64, m64, l64 = CN.head_stats(Xi, W, b)
        arg, m, lse = run_head(Xi, W, b)
        want_dev = CN.collapse(arg[0], 0)
        assert np.array_equal(out[i]["tokens"], want_dev[0]) and np.array_equal(out[i]["start"], want_dev[1]) and np.array_equal(out[i]["length"], want_dev[2])
        if (CN.top2_gap(z) > 2 * CN.delta_z(Xi, W, b).max(axis=1)).all():
            w64 = CN.greedy(a64, m64, l64, 0)
            assert np.array_equal(out[i]["tokens"], w64[0])
            tol = CN.delta_z(Xi, W, b).max(axis=1) + CN.delta_lse(Xi, W, b, l64)
            for k, (s, n) in enumerate(zip(w64[1], w64[2])):
                worst = max(worst, abs(out[i]["logprob"][k] - w64[3][k]) / tol[s:s + n].max())
    print(f"greedy logprob: {worst:.3g} of bound 1 + 2")
    record_margin(worst, 1.0)


# ---- the public score / align ----
def test_public_score_and_align(record_margin):
    """bounds 3 + 4 on (T, V, L, D) = (349, 32, 60, 1024) and (128, 4099, 40, 136); a guarded bad label gives +inf through the C ABI"""
    from encoder.ctc import CTCHead
    from lds import native
    worst = 0.0
    for T, V, L, D in ((349, 32, 60, 1024), (128, 4099, 40, 136)):
        X, W, b = make_head(T + 30, V, D, seed=T)
        rng = np.random.default_rng(T + 1)
        labels = [rng.integers(1, V, L), rng.integers(1, V, L // 2)]
        labels[0][5] = labels[0][4]
        lens = [T, T - 17]
        Xb = np.stack([X[:T], X[30:T + 30]])
        Xb[1, lens[1]:] = np.nan
        head = CTCHead(W, b, blank=0)
        nll = head.score(dev(Xb), lens, labels).cpu().numpy()
        al = head.align(dev(Xb), lens, labels)
        for i in range(2):
            Xi = Xb[i, :lens[i]]
            z, _, _, l64 = CN.head_stats(Xi, W, b)
            E = CN.emissions(z - l64[:, None], labels[i], 0)
            ref, A = CN.forward(E, labels[i])
            opt = CN.viterbi(E, labels[i])[0]
            dE = float((CN.delta_z(Xi, W, b).max(axis=1) + CN.delta_lse(Xi, W, b, l64)).max())
            bound = CN.bound3(lens[i], A) + lens[i] * dE
            path = al[i]["frame_label"]
            assert len(path) == lens[i] and CN.path_states_valid(path, len(labels[i])) and CN.path_respects_repeats(path, labels[i])
            f = max(abs(nll[i] - ref), abs(al[i]["score"] - opt), abs(CN.path_score(E, path) - opt)) / bound
            print(f"public T={T} V={V} L={len(labels[i])} D={D}: nll {nll[i]:.6g} vs {ref:.6g}, Viterbi {al[i]['score']:.6g} vs {opt:.6g}: {f:.3g} of bounds 3 + 4")
            worst = max(worst, f)
    record_margin(worst, 1.0)
    # the kernel's guard (the Python surface refuses such labels before upload): a blank label, one beyond V, a negative one
    T, V, D = 40, 32, 64
    X, W, b = make_head(3 * T, V, D, seed=9)
    lab = np.array([[3, 0, 5], [3, 40, 5], [3, -2, 5], [3, 4, 5]], dtype=np.int64)
    Xb = np.concatenate([X, X[:T]]).reshape(4, T, D)
    nll = native.ctc_score(dev(Xb), [T] * 4, dev(W), dev(b), 0, dev(lab), [3] * 4).cpu().numpy()
    assert (nll[:3] == np.inf).all() and np.isfinite(nll[3])
    ps, fl, seg, _ = (t.cpu().numpy() for t in native.ctc_align(dev(Xb), [T] * 4, dev(W), dev(b), 0, dev(lab), [3] * 4))
    assert (ps[:3] == -np.inf).all() and (seg[:3] == -1).all() and (fl[:3] == -1).all() and np.isfinite(ps[3])


# ---- end to end: audio -> native encoder -> CTCHead against transformers' *ForCTC ----
TOL = 2e-5      # the encoder tests' tolerance (x absmax): the head adds one D-length dot product to a stack already held to that


def _fixture_encoder(model):
    """the fixture's encoder (tests/golden/make_ctc_fixtures.py: the XLSR / WavLM-Base+ fixture weights, 2 layers) and its head"""
    import w2v_numpy as wnp
    import wavlm_numpy as lnp
    from encoder.ctc import CTCHead
    from lds import arch
    from tools.tools import Audio2xlsr_53_56k, WavLMUnits
    if model == "xlsr":
        dims = dict(arch.XLSR_53_DIMS, n_layer=wnp.FIXTURE_LAYERS)
        enc = Audio2xlsr_53_56k(device="cuda", dims=dims, state=arch.w2v_init_state(dims, wnp.FIXTURE_SEED))
    else:
        dims = lnp.dims_of("base", arch)
        enc = WavLMUnits("wavlmbase+", device="cuda", dims=dims, state=arch.wavlm_init_state(dims, lnp.FIXTURE_SEED))
    CTCHead.check_source(enc)
    return enc, CTCHead.synthetic(dims["n_state"], {"xlsr": 32, "wavlm": 33}[model], seed=0, blank=0)


_E2E = {}


def _end_to_end_run(model):
    """both fixture clips (3 and 128 frames) as one ragged batch through the native encoder, once per model"""
    if model not in _E2E:
        import w2v_numpy as wnp
        from lds import init_weights
        enc, head = _fixture_encoder(model)
        clips = [wnp.make_clip(i, init_weights.uniform) for i in (1, 2)]
        audio = np.zeros((2, len(clips[1])), dtype=np.float32)
        for b, c in enumerate(clips):
            audio[b, :len(c)] = c
        units, n_frames = enc.encode_ragged(dev(audio), [len(c) for c in clips])
        n_frames = [int(n) for n in n_frames]
        assert n_frames == [3, 128]
        _E2E[model] = (head, units, n_frames)
    return _E2E[model]


@pytest.mark.parametrize("model", ["xlsr", "wavlm"])
def test_end_to_end_logprobs_and_greedy_against_transformers(model, golden, record_margin):
    """log-probs within TOL x absmax of the model in float64, greedy ids equal outside the gap frames"""
    fx = golden("ctc.npz")
    head, units, n_frames = _end_to_end_run(model)
    lp = head.log_probs(units, n_frames).cpu().numpy()
    arg = run_head(units.cpu().numpy(), head._w.numpy(), head._b.numpy(), n_frames=n_frames)[0]
    greedy = head.greedy(units, n_frames)
    worst = 0.0
    for b, i in enumerate((1, 2)):
        key, T = f"{model}.clip{i}", n_frames[b]
        ref, absmax, inside = fx[f"{key}.logprobs"].astype(np.float64), float(fx[f"{key}.absmax"]), fx[f"{key}.inside"]
        e = float(np.abs(lp[b, :T] - ref).max() / absmax)
        print(f"{key}: log-probs max |native - ref64| / absmax {e:.3e} (the model's own fp32 gap {float(fx[f'{key}.gap']):.2e}); frames inside the gap {int(inside.sum())}")
        worst = max(worst, e)
        assert (lp[b, T:] == 0).all()
        assert np.array_equal(arg[b, :T][~inside], fx[f"{key}.ids"][~inside])
        assert np.array_equal(greedy[b]["tokens"], CN.collapse(arg[b, :T], 0)[0])
        if not inside.any():
            assert np.array_equal(greedy[b]["tokens"], fx[f"{key}.greedy"])
    record_margin(worst, TOL)


@pytest.mark.parametrize("model", ["xlsr", "wavlm"])
def test_end_to_end_score_against_transformers(model, golden, record_margin):
    """score = HF's loss (labels of length 0, 1, 40; +inf where they do not fit) within bounds 3 + 4 plus the log-prob tolerance times T"""
    fx = golden("ctc.npz")
    head, units, n_frames = _end_to_end_run(model)
    worst = 0.0
    Xs = units.cpu().numpy().astype(np.float64)
    W, bias = head._w.numpy(), head._b.numpy()
    for L in (0, 1, 40):
        labels = [fx[f"{model}.clip{i}.labels{L}"] for i in (1, 2)]
        nll = head.score(units, n_frames, labels).cpu().numpy()
        for b, i in enumerate((1, 2)):
            key, T = f"{model}.clip{i}", n_frames[b]
            want = float(fx[f"{key}.loss{L}"])
            if np.isinf(want):
                assert nll[b] == np.inf
                continue
            ref = fx[f"{key}.logprobs"].astype(np.float64)
            _, A = CN.forward(CN.emissions(ref, labels[b], 0), labels[b])
            Xb = Xs[b, :T]
            l64 = CN.head_stats(Xb, W, bias)[3]
            dE = float((CN.delta_z(Xb, W, bias).max(axis=1) + CN.delta_lse(Xb, W, bias, l64)).max())
            bound = CN.bound3(T, A) + T * dE + TOL * float(fx[f"{key}.absmax"]) * T
            print(f"{key} L={L}: score {nll[b]:.7g} vs HF's loss {want:.7g} ({abs(nll[b] - want) / bound:.3g} of the bound)")
            worst = max(worst, abs(nll[b] - want) / bound)
    record_margin(worst, 1.0)


# ---- the tool ----
def test_tool_three_subcommands(tmp_path):
    """tools/ctc_eval.py --synthetic on two short clips (one a 22.05 kHz .wav: resampled on the device): well-formed files, and score of a clip
    against its own greedy transcript yields CER 0"""
    import importlib.util
    import wave
    spec = importlib.util.spec_from_file_location("ctc_eval", os.path.join(ROOT, "tools", "ctc_eval.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rng = np.random.default_rng(3)
    clips = tmp_path / "clips"
    clips.mkdir()
    np.save(clips / "a.npy", (rng.standard_normal(9000) * 0.1).astype(np.float32))
    with wave.open(str(clips / "b.wav"), "wb") as w:
        w.setnchannels(1), w.setsampwidth(2), w.setframerate(22050)
        w.writeframes((rng.standard_normal(7000) * 3000).astype(np.int16).tobytes())
    common = [str(clips), "--synthetic", "--layers", "1", "--encoder", "xlsr_53_56k", "--vocab", "32"]
    out = tool.main(["transcribe"] + common + ["--out", str(tmp_path / "tr")])
    recs = {n: json.load(open(os.path.join(out, n + ".json"))) for n in ("a", "b")}
    for n, r in recs.items():
        k = len(r["tokens"])
        assert r["text"] is None and k > 0 and r["n_frames"] > 0 and all(len(r[f]) == k for f in ("start", "length", "start_s", "end_s", "logprob"))
        assert all(0 < t < 32 for t in r["tokens"]) and all(a < b for a, b in zip(r["start"], r["start"][1:])) and all(v <= 0 for v in r["logprob"])
        assert r["start"][-1] + r["length"][-1] <= r["n_frames"]
        np.save(clips / f"{n}.labels.npy", np.array(r["tokens"], dtype=np.int64))
    assert recs["a"]["n_frames"] == (9000 - 400) // 320 + 1
    out = tool.main(["score"] + common + ["--out", str(tmp_path / "sc")])
    sc = json.load(open(os.path.join(out, "scores.json")))
    assert set(sc["clips"]) == {"a", "b"} and sc["mean"]["cer"] == 0.0
    for n, s in sc["clips"].items():
        assert s["cer"] == 0.0 and s["L"] == len(recs[n]["tokens"]) and 0 < s["nll"] < 1e4 and abs(s["nll_per_label"] - s["nll"] / s["L"]) < 1e-9
    out = tool.main(["align"] + common + ["--out", str(tmp_path / "al")])
    for n, r in recs.items():
        al = json.load(open(os.path.join(out, n + ".align.json")))
        assert al["score"] < 0 and [s["label"] for s in al["segments"]] == r["tokens"]
        assert all(s["start_s"] < s["end_s"] <= r["n_frames"] * 0.02 + 1e-9 and s["logprob"] <= 0 for s in al["segments"])
        assert all(a["end_s"] <= b["start_s"] + 1e-9 for a, b in zip(al["segments"], al["segments"][1:]))
