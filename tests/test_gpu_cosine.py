"""The cosine metric on a real MI355X (csrc/kmeans.hip and csrc/knn.hip through lds.native, cluster.kmeans.KMeansCosineGPU,
cluster.index.UnitsIndex(metric="cosine") and the command-line tools) against the float64 oracle of tests/cosine_numpy.py and the reference's
own KMeansGPU(mode="cosine") (tests/golden/kmeans_cosine.npz): exact indices, similarities and ties on the power-of-two lattice (slabs,
splits, scaled copies), the reference's labels on the scaled blobs, the a-priori bounds on Gaussian inputs, both weightings of the blend,
degenerate rows, bit-for-bit invariances, the limits, the Lloyd step and the fit, the IVF, and the tool chain (kNN-VC's recipe)."""
import ctypes as ct
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import cosine_numpy as CN
import kmeans_numpy as KM
import knn_numpy as KN
from conftest import ROOT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NAN_WORD, X7F_WORD = 0x7FC00000, 0x7F7F7F7F
TOL = 2e-5      # the project's per-kernel tolerance (relative to the abs-max of the compared tensor)
SPEEDUP = 250


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()      # (a copy: the shared inputs are read-only)


def bits(t):
    return t.contiguous().view(torch.int32)


def cos_index(P, **kw):
    from cluster.index import UnitsIndex
    return UnitsIndex(np.array(P), metric="cosine", **kw)


def assign(X, C, **kw):
    from lds import native
    Cd = dev(C)
    return native.kmeans_assign(dev(X), Cd, native.kmeans_prepare(Cd, "cosine"), metric="cosine", **kw)


@pytest.fixture(scope="module")
def fx(golden):
    return golden("kmeans_cosine.npz")


@functools.lru_cache(maxsize=None)
def gaussian(case):
    """(X, P, the oracle's idx, its similarities): computed once, shared, never written to"""
    N, M, D, k = case
    X, P = CN.gaussian_case(N, M, D)
    out = (X, P) + CN.search64(X, P, k)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def gaussian_index(case):
    return cos_index(gaussian(case)[1])


def forced_search(X, P, k, slab_rows, splits, fill=None):
    """lds_test_knn_search_metric: the pool cut into slabs of slab_rows and `splits` ranges of pool blocks"""
    from lds import native
    Pd = dev(P)
    ws = torch.empty(2 * (splits * len(X) * 8 * 4 + 256), dtype=torch.uint8, device="cuda")
    if fill is not None:
        native.debug_fill(ws, fill)
    return native.knn_search(dev(X), Pd, native.knn_prepare(Pd, "cosine"), k, ws=ws, slab_rows=slab_rows, splits=splits, metric="cosine")


def exact(t, want):
    return np.array_equal(t.cpu().numpy().astype(np.float64), want)


# ---- the lattice: every score and every similarity exact in fp32, so indices, values and ties are the oracle's ----
@pytest.mark.parametrize("case", CN.LATTICE, ids=lambda c: "x".join(map(str, c)))
def test_cosine_lattice_exact(case):
    N, M, D, k = case
    X, P = CN.lattice_case(N, M, D)
    want, sim = CN.search64(X, P, k)
    idx, sc = cos_index(P).search(dev(X), k=k)
    assert idx.dtype == torch.int64 and idx.shape == (N, k) and np.array_equal(idx.cpu().numpy(), want) and exact(sc, sim)
    assert (np.diff(sim, axis=1) == 0).sum() >= N // 2      # exact ties inside the lists: the lower index came first
    lab, best = assign(X, P, return_best=True)
    assert np.array_equal(lab.cpu().numpy(), want[:, 0]) and exact(best, sim[:, 0])
    y, ri, dist = cos_index(P).retrieve(dev(X), k=k, ratio=0.5, return_neighbours=True, weights="uniform")
    assert np.array_equal(ri.cpu().numpy(), want)
    assert exact(dist, np.maximum(1.0 - sim, float(np.float32(CN.FLOOR))))      # 1 - cos, exact on the lattice too; 0 takes the floor
    assert np.array_equal(y.cpu().numpy().astype(np.float64), CN.blend64(X, P, want, 0.5, "uniform")[0])      # multiples of 1/16 averaged: exact


@pytest.mark.parametrize("splits", [1, 2, 3])
@pytest.mark.parametrize("M", [333, 261])      # three pool blocks of 128, 128 and 77 or 5 rows: with 3 splits the last holds fewer than k = 8 rows
def test_cosine_lattice_slabs_and_splits(M, splits):
    X, P = CN.lattice_case(129, M, 8)
    want, sim = CN.search64(X, P, 8)
    idx, sc = forced_search(X, P, 8, 128, splits, fill=NAN_WORD)
    assert np.array_equal(idx.cpu().numpy(), want) and exact(sc, sim)


@pytest.mark.parametrize("how", ["library", "slabs_128_splits_3", "slabs_256_splits_2"])
def test_cosine_lattice_scaled_copies_tie(how):
    """every pool row reappears scaled by 2 and by 4, 100 rows apart: the copies' cosine scores are equal bit for bit (the row constants are
    powers of two) and they come lowest index first, across blocks, slabs and splits"""
    X, P = CN.lattice_case(130, 100, 24)
    P3 = np.concatenate([P, 2 * P, 4 * P])
    want, sim = CN.search64(X, P3, 8)
    if how == "library":
        idx, sc = cos_index(P3).search(dev(X), k=8)
    else:
        idx, sc = forced_search(X, P3, 8, int(how.split("_")[1]), int(how.split("_")[3]))
    assert np.array_equal(idx.cpu().numpy(), want) and exact(sc, sim)
    full = CN.sims(X, P3)      # the oracle itself: the three copies of every row tie exactly, so every list opens with an original
    assert np.array_equal(full[:, :100], full[:, 100:200]) and np.array_equal(full[:, :100], full[:, 200:]) and (want[:, 0] < 100).all()
    assert (sim[:, 0] == sim[:, 2]).all()      # at least three rows tie at the top of every list: the index alone orders them
    lab = assign(X, P3)
    assert np.array_equal(lab.cpu().numpy(), want[:, 0])


# ---- the reference's labels ----
@pytest.mark.parametrize("name", list(CN.BLOBS))
def test_cosine_assign_equals_the_reference(fx, name, record_margin):
    K, D, N, _, B, lens = CN.BLOBS[name]
    C, X, _ = CN.scaled_blobs(int(fx[f"{name}.seed"]), K, D, N)
    ref = fx[f"{name}.ref"].astype(np.int64)
    if B:
        T = N // B
        Xr = X.reshape(B, T, D).copy()
        for b, n in enumerate(lens):
            Xr[b, n:] = np.nan
        lab, best = assign(Xr, C, return_best=True, lengths=list(lens), pad_id=-7)
        lab, best = lab.cpu().numpy(), best.cpu().numpy()
        keep = np.arange(T)[None, :] < np.array(lens)[:, None]
        assert lab.shape == (B, T) and (lab[~keep] == -7).all() and (best[~keep] == 0).all()
        assert np.array_equal(lab[keep], ref.reshape(B, T)[keep])
        lab, best, keep = lab.reshape(-1), best.reshape(-1), keep.reshape(-1)
    else:
        lab, best = assign(X, C, return_best=True)
        lab, best, keep = lab.cpu().numpy(), best.cpu().numpy(), np.ones(N, bool)
        assert np.array_equal(lab, ref)
        assert int((assign_l2(X, C) != lab).sum()) >= N // 5      # the Euclidean kernel does not pass for the cosine one here
    true = CN.assign64(X, C)[1]
    worst = float(np.abs(best[keep] - true[keep]).max() / CN.sim_bound(D))
    print(f"{name}: |best - cos64| / bound {worst:.3g}")
    record_margin(worst, 1.0)


def assign_l2(X, C):
    from lds import native
    Cd = dev(C)
    return native.kmeans_assign(dev(X), Cd, native.kmeans_prepare(Cd)).cpu().numpy()


def test_cosine_max_sim_and_get_cluster_result(fx):
    import types

    import cluster
    from cluster.kmeans import KMeansCosineGPU
    name = "odd_333x136"
    K, D, N = CN.BLOBS[name][:3]
    C, X, _ = CN.scaled_blobs(int(fx[f"{name}.seed"]), K, D, N)
    v, i = KMeansCosineGPU(K).max_sim(torch.from_numpy(X), torch.from_numpy(C))
    assert np.array_equal(i.cpu().numpy(), fx[f"{name}.ref"]) and np.abs(v.cpu().numpy() - fx[f"{name}.ref_sim"]).max() <= 2 * CN.sim_bound(D)
    model = types.SimpleNamespace(cluster_centers_=C)
    got = cluster.get_cluster_result(model, dev(X), metric="cosine")
    assert torch.equal(got, i) and not torch.equal(cluster.get_cluster_result(model, dev(X)), i)


# ---- Gaussian inputs: the a-priori bounds ----
@functools.lru_cache(maxsize=None)
def gaussian_search(case):
    """the GPU's lists on a Gaussian case: (idx numpy, reported similarities numpy, their true float64 similarities)"""
    X, P = gaussian(case)[:2]
    idx, score = gaussian_index(case).search(dev(X), k=case[3])
    idx = idx.cpu().numpy()
    return idx, score.cpu().numpy(), CN.sim64(X, P, idx)


@pytest.mark.parametrize("case", CN.GAUSSIAN, ids=lambda c: "x".join(map(str, c)))
def test_cosine_gaussian_within_search_bound(case, record_margin):
    """every returned neighbour's true (float64) similarity lies at most 2 (D + 4) 2^-24 below the oracle's of the same rank; indices distinct
    and inside [0, M); similarities in descending order"""
    N, M, D, k = case
    want, sim_want = gaussian(case)[2:]
    idx, score, true = gaussian_search(case)
    assert idx.min() >= 0 and idx.max() < M and all(len(set(r)) == k for r in idx)
    worst = float((sim_want - true).max() / CN.search_bound(D))
    print(f"{case}: worst shortfall / bound {worst:.3g}; rows whose list differs from float64's: {int((idx != want).any(1).sum())} of {N}")
    record_margin(worst, 1.0)
    assert (np.diff(score, axis=1) <= 0).all()


@pytest.mark.parametrize("case", CN.GAUSSIAN, ids=lambda c: "x".join(map(str, c)))
def test_cosine_gaussian_reported_similarity(case, record_margin):
    """the reported similarity lies within (D + 4) 2^-24 of the true one of the row it names"""
    idx, score, true = gaussian_search(case)
    worst = float(np.abs(score - true).max() / CN.sim_bound(case[2]))
    print(f"{case}: |score - cos64| / bound {worst:.3g}")
    record_margin(worst, 1.0)


BLENDS = [(4, 1.0, "uniform"), (8, 0.5, "inverse_square"), (1, 0.75, "uniform"), (3, 0.25, "inverse_square")]


@functools.lru_cache(maxsize=None)
def gaussian_blend(k, ratio, weights):
    """the GPU's blend on CN.GAUSSIAN[0] and the oracle on the GPU's own neighbours: (y, idx, dist, y64, d64) as numpy"""
    case = CN.GAUSSIAN[0]
    X, P = gaussian(case)[:2]
    y, idx, dist = gaussian_index(case).retrieve(dev(X), k=k, ratio=ratio, return_neighbours=True, weights=weights)
    idx = idx.cpu().numpy()
    y64, d64, _ = CN.blend64(X, P, idx, ratio, weights)
    return y.cpu().numpy(), idx, dist.cpu().numpy().astype(np.float64), y64, d64


@pytest.mark.parametrize("k,ratio,weights", BLENDS)
def test_cosine_blend_on_own_neighbours(k, ratio, weights, record_margin):
    case = CN.GAUSSIAN[0]
    X, P = gaussian(case)[:2]
    y, idx, dist, y64, d64 = gaussian_blend(k, ratio, weights)
    worst = float(np.abs(y - y64).max() / CN.blend_bound(X, P, d64.min()))
    print(f"k {k} ratio {ratio} {weights}: |y - y64| / bound {worst:.3g}")
    record_margin(worst, 1.0)
    assert np.array_equal(idx, gaussian_index(case).search(dev(X), k=k)[0].cpu().numpy())


@pytest.mark.parametrize("k,ratio,weights", BLENDS)
def test_cosine_blend_distances(k, ratio, weights, record_margin):
    """the distances the weights were formed from: 1 - cos of the GPU's own neighbours within cosine_numpy.dist_bound"""
    D = CN.GAUSSIAN[0][2]
    y, idx, dist, y64, d64 = gaussian_blend(k, ratio, weights)
    worst = float((np.abs(dist - d64) / (CN.dist_bound(D, d64) * d64)).max())
    print(f"k {k} ratio {ratio} {weights}: |d - d64| / bound {worst:.3g}")
    record_margin(worst, 1.0)


def test_cosine_blend_ends_pool_rows_and_l2_uniform(record_margin):
    from cluster.index import UnitsIndex
    case = CN.GAUSSIAN[0]
    X, P = gaussian(case)[:2]
    ix, Xd = gaussian_index(case), dev(X)
    for weights in ("uniform", "inverse_square"):
        y0 = ix.retrieve(Xd, k=8, ratio=0.0, weights=weights)
        assert torch.equal(bits(y0), bits(Xd))                                   # ratio 0: x bit for bit
    rows = np.array([0, 127, 128, 2500, 4999])
    for weights in ("uniform", "inverse_square"):
        yq, iq, dq = ix.retrieve(dev(P[rows]), k=1, ratio=1.0, return_neighbours=True, weights=weights)
        assert np.array_equal(iq[:, 0].cpu().numpy(), rows) and torch.equal(bits(yq), bits(dev(P[rows])))      # the ORIGINAL row, not a normalised one
        assert (dq[:, 0] == float(np.float32(CN.FLOOR))).all()                  # the same row constant on both sides: d = 0 takes the floor
    # Euclidean distances with uniform weights against their own oracle
    l2 = UnitsIndex(np.array(P))
    y, idx, dist = l2.retrieve(Xd, k=4, ratio=0.5, return_neighbours=True, weights="uniform")
    idx = idx.cpu().numpy()
    assert np.array_equal(idx, l2.search(Xd, k=4)[0].cpu().numpy())
    y64, d64, _ = CN.blend64(X, P, idx, 0.5, "uniform", metric="l2")
    worst = float(np.abs(y.cpu().numpy() - y64).max() / KN.blend_bound(X, P))
    record_margin(worst, 1.0)
    assert (np.abs(dist.cpu().numpy() - d64) <= (X.shape[1] + 4) * 2.0 ** -24 * d64).all()
    # and l2 with inverse_square through the new argument is the call without it, bit for bit
    a, b = l2.retrieve(Xd, k=8, ratio=0.5, weights="inverse_square"), l2.retrieve(Xd, k=8, ratio=0.5)
    assert torch.equal(bits(a), bits(b))


# ---- degenerate rows ----
def test_cosine_zero_rows_nan_rows_and_extreme_scales(fx):
    X, P = CN.lattice_case(40, 16, 8)
    P = P.copy()
    P[5] = 0.0
    ix = cos_index(P)
    idx, sc = ix.search(dev(X), k=8)
    full_idx, full_sc = ix.search(dev(X), k=8)
    want, sim = CN.search64(X, P, 8)
    assert np.array_equal(idx.cpu().numpy(), want) and exact(sc, sim) and torch.isfinite(sc).all()
    lab, best = assign(X, P, return_best=True)
    allsim = CN.sims(X, P)
    assert (allsim[:, 5] == 0).all() and np.array_equal(lab.cpu().numpy(), allsim.argmax(1)) and torch.isfinite(best).all()
    neg = np.flatnonzero(allsim.max(1) <= 0)      # rows whose best similarity is 0: the zero row competes, the lowest index among the zeros wins
    assert all(lab[n] == np.flatnonzero(allsim[n] == allsim[n].max())[0] for n in neg)
    # a zero query: every score is 0, so the k lowest indices, similarity 0, d = 1/2 (0 against a zero pool row)
    Xz = np.concatenate([np.zeros((1, 8), np.float32), X[:3]])
    y, zi, zd = ix.retrieve(dev(Xz), k=8, ratio=1.0, return_neighbours=True, weights="uniform")
    assert np.array_equal(zi[0].cpu().numpy(), np.arange(8)) and torch.isfinite(y).all()
    zd = zd[0].cpu().numpy()
    assert np.array_equal(np.delete(zd, 5), np.full(7, 0.5, np.float32)) and zd[5] == np.float32(CN.FLOOR)
    assert np.array_equal(y[0].cpu().numpy().astype(np.float64), CN.blend64(Xz[:1], P, np.arange(8)[None], 1.0, "uniform")[0][0])
    assert not ix.search(dev(Xz), k=8)[1][0].any()
    # a NaN query: -1 everywhere, -inf scores, no neighbours found; the other rows do not notice
    Xn = X[:5].copy()
    Xn[2, 3] = np.nan
    ni, ns = ix.search(dev(Xn), k=4)
    assert (ni[2] == -1).all() and torch.isneginf(ns[2]).all() and torch.equal(ni[[0, 1, 3, 4]], full_idx[[0, 1, 3, 4], :4])
    for weights in ("uniform", "inverse_square"):
        yn, ri, rd = ix.retrieve(dev(Xn), k=4, ratio=0.5, return_neighbours=True, weights=weights)
        yo = ix.retrieve(dev(X[:5]), k=4, ratio=0.5, weights=weights)
        assert (ri[2] == -1).all() and torch.equal(bits(yn[[0, 1, 3, 4]]), bits(yo[[0, 1, 3, 4]]))
    assert assign(Xn, P).cpu().numpy()[2] == 0
    # rows scaled by 1e-15 and 1e15 label like their unscaled selves (the reference's labels): the order never sees r(x).  Their similarity
    # is the oracle's of the scaled rows -- a row of norm below 1e-12 meets F.normalize's eps and reports (x . c) r(c) 1e12, as the reference does.
    # Centres scaled within the eps-free range leave labels and similarities alone.
    name = "odd_333x136"
    K, D, N = CN.BLOBS[name][:3]
    C, Xb, _ = CN.scaled_blobs(int(fx[f"{name}.seed"]), K, D, N)
    ref = fx[f"{name}.ref"]
    for sx, sc_ in ((1e-15, 1.0), (1e15, 1.0), (1.0, 2.0 ** -20), (1.0, 1e15), (1e15, 2.0 ** -20)):
        Xs, Cs = (Xb * np.float32(sx)).astype(np.float32), (C * np.float32(sc_)).astype(np.float32)
        lab, best = assign(Xs, Cs, return_best=True)
        assert np.array_equal(lab.cpu().numpy(), ref), (sx, sc_)
        l64, b64, _ = CN.assign64(Xs, Cs)
        assert np.array_equal(l64, ref) and (np.abs(best.cpu().numpy() - b64) <= CN.sim_bound(D) * np.maximum(np.abs(b64), 1.0)).all(), (sx, sc_)
        if sx > 1:
            assert np.abs(best.cpu().numpy() - fx[f"{name}.ref_sim"]).max() <= 2 * CN.sim_bound(D)


# ---- invariances ----
def test_cosine_row_alone_in_a_batch_and_ragged():
    case = CN.GAUSSIAN[0]
    X = gaussian(case)[0]
    ix, Xd = gaussian_index(case), dev(X[:129])
    kw = dict(k=4, ratio=1.0, return_neighbours=True, weights="uniform")
    y, idx, dist = ix.retrieve(Xd, **kw)
    sidx, ssc = ix.search(Xd, k=4)
    for n in (0, 31, 64, 127, 128):
        y1, i1, d1 = ix.retrieve(Xd[n:n + 1].contiguous(), **kw)
        assert torch.equal(i1[0], idx[n]) and torch.equal(bits(d1[0]), bits(dist[n])) and torch.equal(bits(y1[0]), bits(y[n])), n
        s1 = ix.search(Xd[n:n + 1].contiguous(), k=4)
        assert torch.equal(s1[0][0], sidx[n]) and torch.equal(bits(s1[1][0]), bits(ssc[n]))
    yb, ib, db = ix.retrieve(dev(np.concatenate([X[200:257], X[:129]])), **kw)      # other rows in front
    assert torch.equal(ib[57:], idx) and torch.equal(bits(db[57:]), bits(dist)) and torch.equal(bits(yb[57:]), bits(y))
    B, T, lengths = 3, 40, (40, 0, 17)
    Xr = np.full((B, T, X.shape[1]), np.nan, np.float32)
    Xr[0], Xr[2, :17] = X[:40], X[40:57]
    yr, ir, dr = ix.retrieve(dev(Xr), lengths=lengths, **kw)
    for got, want in ((yr, y), (dr, dist)):
        assert torch.equal(bits(got[0]), bits(want[:40])) and torch.equal(bits(got[2, :17]), bits(want[40:57]))
        assert not got[1].any() and not got[2, 17:].any()
    assert torch.equal(ir[0], idx[:40]) and torch.equal(ir[2, :17], idx[40:57]) and (ir[1] == -1).all() and (ir[2, 17:] == -1).all()
    base = forced_search(X[:129], gaussian(case)[1], 8, 4992, 1)
    for slab_rows, splits in ((128, 7), (2560, 2)):
        got = forced_search(X[:129], gaussian(case)[1], 8, slab_rows, splits)
        assert torch.equal(got[0], base[0]) and torch.equal(bits(got[1]), bits(base[1])), (slab_rows, splits)
    lab, best = assign(X[:129], gaussian(case)[1][:300], return_best=True)
    l1, b1 = assign(X[77:78], gaussian(case)[1][:300], return_best=True)
    assert l1[0] == lab[77] and torch.equal(bits(b1), bits(best[77:78]))


def test_cosine_repeat_with_nan_in_the_workspace():
    from lds import native
    case = CN.GAUSSIAN[0]
    X, P = gaussian(case)[:2]
    Xd = dev(X)
    pool, h = gaussian_index(case)._device(Xd.device)
    ws = torch.empty(native.knn_workspace_bytes(len(X), len(P), X.shape[1], 8), dtype=torch.uint8, device="cuda")
    C = dev(P[:1000])
    hc = native.kmeans_prepare(C, "cosine")
    kws = torch.empty(native.kmeans_workspace_bytes(len(X), 1000, X.shape[1]) // 4 * 4, dtype=torch.uint8, device="cuda")
    outs = []
    for fill in (None, NAN_WORD, X7F_WORD):
        if fill is not None:
            native.debug_fill(ws, fill)
            native.debug_fill(kws, fill)
        else:
            ws.zero_()
            kws.zero_()
        r = native.knn_retrieve(Xd, pool, h, 8, 0.5, ws=ws, metric="cosine", weights="uniform")
        if fill is not None:
            native.debug_fill(ws, fill)
        s = native.knn_search(Xd, pool, h, 8, ws=ws, metric="cosine")
        a = native.kmeans_assign(Xd, C, hc, return_best=True, ws=kws, metric="cosine")
        outs.append(tuple(r) + tuple(s) + tuple(a))
    for o in outs[1:]:
        assert all(torch.equal(bits(u) if u.dtype == torch.float32 else u, bits(v) if v.dtype == torch.float32 else v) for u, v in zip(o, outs[0]))
    assert torch.isfinite(outs[0][0]).all()


def test_cosine_limits_return_codes_and_enqueue_nothing():
    from lds import native
    L = native.lib()
    N, M, D, k = 37, 300, 16, 4
    X, P = CN.lattice_case(N, M, D)
    Xd, Pd = dev(X), dev(P)
    h = native.knn_prepare(Pd, "cosine")
    need = native.knn_workspace_bytes(N, M, D, k)
    kneed = native.kmeans_workspace_bytes(N, M, D)

    def call(entry, N=N, M=M, D=D, k=k, metric=1, weights=1, ratio=0.5, ws_bytes=need, lengths=None):
        y = torch.full((N, D), 7.0, device="cuda")
        idx = torch.full((N, 8), 7, dtype=torch.int32, device="cuda")
        dist = torch.full((N, 8), 7.0, device="cuda")
        lab = torch.full((N,), 7, dtype=torch.int64, device="cuda")
        hh = torch.full((M,), 7.0, device="cuda")
        ws = torch.zeros(max(ws_bytes, 16), dtype=torch.uint8, device="cuda")
        tail = (idx.data_ptr(), dist.data_ptr(), ws.data_ptr(), ws_bytes, native._stream())
        head = (Xd.data_ptr(), N, Pd.data_ptr(), h.data_ptr(), M, D, k)
        if entry == "search":
            rc = L.lds_knn_search_metric(*head, metric, *tail)
        elif entry == "forced":
            rc = L.lds_test_knn_search_metric(*head, metric, 128, 2, *tail)
        elif entry == "ragged":
            ln = (ct.c_int32 * 1)(*lengths)
            rc = L.lds_knn_retrieve_ragged_metric(Xd.data_ptr(), 1, N, ct.cast(ln, ct.c_void_p), Pd.data_ptr(), h.data_ptr(), M, D, k, metric, weights, ratio,
                                                  y.data_ptr(), *tail)
        elif entry == "retrieve":
            rc = L.lds_knn_retrieve_metric(*head, metric, weights, ratio, y.data_ptr(), *tail)
        elif entry == "prepare":
            rc = L.lds_knn_prepare_metric(Pd.data_ptr(), M, D, metric, hh.data_ptr(), native._stream())
        elif entry == "kprepare":
            rc = L.lds_kmeans_prepare_metric(Pd.data_ptr(), M, D, metric, hh.data_ptr(), native._stream())
        elif entry == "assign":
            rc = L.lds_kmeans_assign_metric(Xd.data_ptr(), N, Pd.data_ptr(), h.data_ptr(), M, D, metric, lab.data_ptr(), dist.data_ptr(), ws.data_ptr(), ws_bytes,
                                            native._stream())
        else:
            raise AssertionError(entry)
        torch.cuda.synchronize()
        untouched = bool((y == 7).all()) and bool((idx == 7).all()) and bool((dist == 7).all()) and bool((lab == 7).all()) and bool((hh == 7).all())
        assert untouched and not bool(ws.any()), "something ran"
        return rc

    err = L.lds_last_error
    for entry in ("search", "forced", "retrieve", "prepare", "kprepare", "assign"):
        wsb = kneed if entry == "assign" else need
        for bad in (2, -1):
            assert call(entry, metric=bad, ws_bytes=wsb) == -1 and b"metric" in err(), entry
        assert call(entry, D=12, ws_bytes=wsb) == -1 and b"D 12" in err(), entry
    for entry in ("search", "forced", "retrieve"):
        assert call(entry, k=9) == -1 and b"k 9" in err()
        assert call(entry, ws_bytes=need - 256 if entry != "forced" else 256) == -2 and b"workspace" in err()
    for bad in (2, -1):
        assert call("retrieve", weights=bad) == -1 and b"weights" in err()
        assert call("ragged", weights=bad, lengths=[N]) == -1 and b"weights" in err()
    assert call("retrieve", ratio=1.5) == -1 and b"ratio" in err()
    assert call("ragged", lengths=[N + 1]) == -1 and b"lengths[0]" in err()
    assert call("assign", ws_bytes=16) == -2 and b"workspace" in err()
    # and the same call inside the limits runs
    assert np.array_equal(cos_index(P).search(Xd, k=k)[0].cpu().numpy(), CN.search64(X, P, k)[0])


# ---- the Lloyd step and the fit ----
def fit_inputs():
    F = CN.FIT
    return CN.scaled_blobs(F["seed"], F["K"], F["D"], F["N"])[1]


def test_cosine_update_step_vs_fixture(fx, record_margin):
    """every iteration of the reference's cosine run on its own: the float64 state in, the cosine assignment compared with the fixture's labels
    (equal wherever the float64 gap exceeds the search bound, inside the bound elsewhere), the step taken on the fixture's labels, the new state
    compared, and r after the update = prepare on the new centres bit for bit"""
    from lds import native
    F = CN.FIT
    X = fit_inputs()
    Xd = dev(X)
    C64, np64 = fx["fit.start"].astype(np.float64), np.ones(F["K"])
    worst_c = worst_n = worst_e = 0.0
    unclear = 0
    for i, lab in enumerate(fx["fit.labels"].astype(np.int64)):
        C32 = C64.astype(np.float32)
        Cd, npd = dev(C32), dev(np64.astype(np.float32))
        h = native.kmeans_prepare(Cd, "cosine")
        got = native.kmeans_assign(Xd, Cd, h, metric="cosine").cpu().numpy()
        if i % 8 == 0 or i == len(fx["fit.labels"]) - 1:      # (the float64 gaps of 6000 x 64 similarities: every eighth iteration and the last)
            l64, _, gap = CN.assign64(X, C32)
            clear = gap > CN.search_bound(F["D"])
            unclear += int((~clear).sum())
            assert np.array_equal(got[clear], l64[clear]), i
            s = CN.sims(X[~clear], C32)
            assert (s.max(1) - s[np.arange(len(s)), got[~clear]] <= CN.search_bound(F["D"])).all(), i
        assert (got != lab).sum() <= 2, i      # the reference's own fp32 labels: all but a row that sits on a tie
        err = native.kmeans_update(Xd, dev(lab), Cd, h, npd, metric="cosine")
        C64n, np64n, e64, _ = KM.lloyd_step64(X, lab, C32, np64.astype(np.float32))
        worst_c = max(worst_c, float(np.abs(Cd.cpu().numpy() - C64n).max() / np.abs(C64n).max()))
        worst_n = max(worst_n, float(np.abs(npd.cpu().numpy() - np64n).max() / np.abs(np64n).max()))
        worst_e = max(worst_e, abs(float(err) - e64) / e64)
        assert torch.equal(bits(h), bits(native.kmeans_prepare(Cd, "cosine"))) and not torch.equal(bits(h), bits(native.kmeans_prepare(Cd)))
        C64, np64 = C64n, np64n
    print(f"cosine update: centroids {worst_c:.2e}, num_points {worst_n:.2e} of abs-max, error {worst_e:.2e} relative; rows inside the bound of a tie: {unclear}")
    record_margin(worst_c, TOL, "centroids")
    record_margin(worst_n, TOL, "num_points")
    record_margin(worst_e, TOL, "error")


def test_cosine_fit_from_captured_start(fx, record_margin):
    from cluster.kmeans import KMeansCosineGPU, KMeansGPU
    F = CN.FIT
    km = KMeansCosineGPU(F["K"], max_iter=F["max_iter"], tol=F["tol"], init=fx["fit.start"], minibatch=10 ** 9)
    assert km.mode == "cosine"
    last = km.fit_predict(torch.from_numpy(fit_inputs()))
    assert km.n_iter_ == len(fx["fit.errors"]), (km.n_iter_, len(fx["fit.errors"]))
    assert last.dtype == torch.int64 and last.is_cuda and np.array_equal(last.cpu().numpy(), fx["fit.labels"][-1].astype(np.int64))
    e = np.abs(np.array(km.errors_) - fx["fit.errors64"]) / fx["fit.errors64"]
    print(f"cosine fit: {km.n_iter_} iterations, worst error-trajectory deviation {e.max():.2e}")
    record_margin(float(np.abs(km.centroids.cpu().numpy() - fx["fit.centroids64"]).max() / np.abs(fx["fit.centroids64"]).max()), TOL)
    # the Euclidean fit from the same start goes elsewhere: the mode is not a label
    ke = KMeansGPU(F["K"], max_iter=3, tol=0.0, init=fx["fit.start"], minibatch=10 ** 9)
    assert not np.array_equal(ke.fit_predict(torch.from_numpy(fit_inputs())).cpu().numpy(), fx["fit.labels"][2].astype(np.int64))


# ---- the IVF in cosine ----
@pytest.mark.parametrize("case", [(129, 8, 8, 8, 3), (127, 257, 24, 4, 5), (128, 1000, 64, 8, 8)], ids=lambda c: "x".join(map(str, c)))
def test_cosine_ivf_all_lists_probed_equals_the_exact_search(case):
    N, M, D, k, L = case
    X, P = CN.lattice_case(N, M, D)
    C = CN.lattice_rows(np.random.default_rng([L, D, 5]), L, D)
    ix = cos_index(P).build_ivf(L, centres=C)
    ivf = CN.ivf_build(P, C)
    assert np.array_equal(ix.ivf["offsets"], ivf[1]) and np.array_equal(ix.ivf["order"], ivf[2]) and np.array_equal(ix.ivf["centres"], ivf[0])
    want, sim = CN.search64(X, P, k)
    idx, sc = ix.search(dev(X), k=k, nprobe=ix.nlist)
    e_idx, e_sc = ix.search(dev(X), k=k)
    assert torch.equal(idx, e_idx) and torch.equal(bits(sc), bits(e_sc)) and np.array_equal(idx.cpu().numpy(), want) and exact(sc, sim)
    a = ix.retrieve(dev(X), k=k, ratio=0.5, return_neighbours=True, nprobe=ix.nlist, weights="uniform")
    b = ix.retrieve(dev(X), k=k, ratio=0.5, return_neighbours=True, weights="uniform")
    assert torch.equal(a[1], b[1]) and torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[2]), bits(b[2]))
    # one list probed: the oracle's candidates, its order, its -1 / -inf fill
    w1, s1 = CN.ivf_search(X, P, k, ivf, 1)
    i1, c1 = ix.search(dev(X), k=k, nprobe=1)
    assert np.array_equal(i1.cpu().numpy(), w1) and exact(c1, s1)
    assert np.array_equal(ix.probe_lists(dev(X), 1).cpu().numpy(), CN.ivf_probe(X, ivf[0], 1))


def test_cosine_ivf_5000_rows_32_lists(record_margin):
    """Gaussian pool of 5000 rows, 32 fitted-free Gaussian centres, nprobe 4: the lists probed are probe_lists', the candidates exactly the
    rows of those lists, and among them the result is the oracle's within the search bound"""
    N, M, D, k = CN.GAUSSIAN[0]
    X, P = gaussian(CN.GAUSSIAN[0])[:2]
    C = np.random.default_rng([32, D, 3]).standard_normal((32, D)).astype(np.float32)
    ix = cos_index(P).build_ivf(32, centres=C)
    assert ix.nlist == 32
    # the lists themselves: every row sits in a list whose centre is the best within the bound
    list_of = np.empty(M, np.int64)
    list_of[ix.ivf["order"]] = np.repeat(np.arange(32), np.diff(ix.ivf["offsets"]))
    s = CN.sims(P, ix.ivf["centres"])
    assert (s.max(1) - s[np.arange(M), list_of] <= CN.search_bound(D)).all() and (np.diff(ix.ivf["order"][: ix.ivf["offsets"][1]]) > 0).all()
    probe = ix.probe_lists(dev(X), 4).cpu().numpy()
    sp = CN.sims(X, ix.ivf["centres"])
    assert (np.sort(sp, axis=1)[:, ::-1][:, :4] - np.take_along_axis(sp, probe, 1) <= CN.search_bound(D)).all() and all(len(set(r)) == 4 for r in probe)
    idx, sc = ix.search(dev(X), k=k, nprobe=4)
    idx = idx.cpu().numpy()
    cand = (list_of[None, :, None] == probe[:, None, :]).any(2)
    assert idx.min() >= 0 and np.take_along_axis(cand, idx, 1).all() and all(len(set(r)) == k for r in idx)      # candidates only
    allsim = CN.sims(X, P)
    best = -np.sort(-np.where(cand, allsim, -np.inf), axis=1)[:, :k]      # the oracle over exactly those candidates
    true = CN.sim64(X, P, idx)
    worst = float((best - true).max() / CN.search_bound(D))
    print(f"ivf 5000 x 32, nprobe 4: worst shortfall / bound {worst:.3g}")
    record_margin(worst, 1.0)
    assert np.abs(sc.cpu().numpy() - true).max() <= CN.sim_bound(D)
    yi = ix.retrieve(dev(X), k=k, ratio=0.5, return_neighbours=True, nprobe=4, weights="uniform")
    assert np.array_equal(yi[1].cpu().numpy(), idx)
    # and a repeat over a workspace full of NaN, then of 0x7f bytes, is bit-identical
    from lds import native
    Xd = dev(X)
    pool, h = ix._device(Xd.device)
    on = ix._device_ivf(Xd.device)
    ws = torch.empty(native.ivf_workspace_bytes(N, M, D, k, 32, 4), dtype=torch.uint8, device="cuda")
    for fill in (NAN_WORD, X7F_WORD):
        native.debug_fill(ws, fill)
        si, ss = native.ivf_search(Xd, pool, h, k, on, 4, ws=ws, metric="cosine")
        native.debug_fill(ws, fill)
        ry, ri, rd = native.ivf_retrieve(Xd, pool, h, k, 0.5, on, 4, ws=ws, metric="cosine", weights="uniform")
        assert np.array_equal(si.cpu().numpy(), idx) and torch.equal(bits(ss), bits(sc))
        assert torch.equal(bits(ry), bits(yi[0])) and torch.equal(ri.to(torch.int64), yi[1]) and torch.equal(bits(rd), bits(yi[2]))


def test_cosine_ivf_short_probe_blends_over_the_rows_found():
    """one probed list that holds fewer than k rows: -1 / -inf behind its rows, and the uniform blend is the plain mean of the rows found"""
    X, P = CN.lattice_case(129, 8, 8)
    C = CN.lattice_rows(np.random.default_rng([3, 8, 5]), 3, 8)
    ix = cos_index(P).build_ivf(3, centres=C)
    ivf = (ix.ivf["centres"], ix.ivf["offsets"], ix.ivf["order"])
    want, sim = CN.ivf_search(X, P, 8, ivf, 1)
    assert (want == -1).any() and (want[:, 0] >= 0).all()
    idx, sc = ix.search(dev(X), k=8, nprobe=1)
    assert np.array_equal(idx.cpu().numpy(), want) and exact(sc, sim) and np.array_equal(want == -1, np.isneginf(sc.cpu().numpy()))
    y, ri, rd = ix.retrieve(dev(X), k=8, ratio=1.0, return_neighbours=True, nprobe=1, weights="uniform")
    y64, d64, w64 = CN.blend64(X, P, want, 1.0, "uniform")
    assert np.array_equal(ri.cpu().numpy(), want) and np.abs(y.cpu().numpy() - y64).max() <= 4 * 2.0 ** -24 * np.abs(P).max()
    found = (want >= 0).sum(1)
    assert np.allclose(w64.sum(1), 1.0) and (found < 8).any() and np.array_equal((w64 > 0).sum(1), found)
    one = np.flatnonzero(found == 1)
    if len(one):
        assert np.array_equal(y.cpu().numpy()[one], P[want[one, 0]])      # a single row found: that row itself


# ---- end to end ----
def test_cosine_tools_knn_vc_recipe(tmp_path):
    """train_units_index.py --metric cosine --nlist, then infer_svc.py --index .. --index_k 4 --index_weights uniform --index_ratio 1.0"""
    import importlib.util

    import infer_svc
    from cluster.index import UnitsIndex
    spec = importlib.util.spec_from_file_location("train_units_index", os.path.join(ROOT, "tools", "train_units_index.py"))
    train_units_index = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train_units_index)
    udir = tmp_path / "units"
    udir.mkdir()
    rng = np.random.default_rng(8)
    for i in range(3):
        np.save(udir / f"clip{i}.npy", rng.standard_normal((150, 64)).astype(np.float32))
    out = tmp_path / "cos_index.pt"
    torch.manual_seed(0)
    train_units_index.main([str(udir), "-o", str(out), "--metric", "cosine", "--nlist", "4", "--nlist_iter", "5"])
    ix = UnitsIndex.load(out)
    assert ix.metric == "cosine" and len(ix) == 450 and 1 <= ix.nlist <= 4
    args = ["--synthetic", "--synthetic_width", "64", "--synthetic_layers", "1", "--synthetic_seconds", "4", "-sr", "22050", "-s", str(SPEEDUP), "--min_len", "500"]
    a = infer_svc.main(args + ["-o", str(tmp_path / "a.npy"), "--index", str(out), "--index_k", "4", "--index_weights", "uniform", "--index_ratio", "1.0"])
    b = infer_svc.main(args + ["-o", str(tmp_path / "b.npy")])
    c = infer_svc.main(args + ["-o", str(tmp_path / "c.npy"), "--index", str(out), "--index_k", "4", "--index_weights", "uniform", "--index_ratio", "1.0",
                               "--index_nprobe", "2"])
    assert a.shape == b.shape == c.shape and np.isfinite(a).all() and np.isfinite(c).all() and np.abs(a).max() > 0 and not np.array_equal(a, b)
    # --max_rows: the reduction is cosine k-means, and the file says so
    red = tmp_path / "reduced.pt"
    torch.manual_seed(0)
    train_units_index.main([str(udir), "-o", str(red), "--metric", "cosine", "--max_rows", "100", "--reduce_to", "16", "--max_iter", "5"])
    rx = UnitsIndex.load(red)
    assert rx.metric == "cosine" and rx.reduced and len(rx) == 16 and rx.source_rows == 450


def test_cosine_tools_train_codebook_and_extract_tokens_cosine(tmp_path):
    import cluster
    from lds import native
    C0, X, _ = CN.scaled_blobs(17, 16, 64, 1200, 0.3)
    udir = tmp_path / "units"
    udir.mkdir()
    cuts = [0, 100, 333, 700, 1200]
    for i in range(4):
        np.save(udir / f"clip{i}.npy", X[cuts[i]:cuts[i + 1]])
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    ck = tmp_path / "semantic_codebook.pt"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_codebook.py"), str(udir), "--out", str(ck), "--n_clusters", "16",
                        "--max_iter", "20", "--mode", "cosine"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    model = cluster.get_cluster_model(str(ck))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "extract_tokens.py"), str(udir), "--codebook", str(ck), "--batch", "3", "--metric", "cosine"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    Cd = dev(model.cluster_centers_.astype(np.float32))
    want = native.kmeans_assign(dev(X), Cd, native.kmeans_prepare(Cd, "cosine"), metric="cosine").cpu().numpy()
    got = np.concatenate([np.load(tmp_path / "semantic_token" / f"clip{i}.npy") for i in range(4)])
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert np.array_equal(want, CN.assign64(X, model.cluster_centers_)[0])      # clear blobs: the float64 cosine labels
    assert (want != model.predict(X)).any()                                     # and not scikit-learn's Euclidean ones


def test_cosine_encode_tokens_takes_the_metric():
    import types

    from encoder.whisper.model import ModelDimensions
    from lds import arch, native
    from tools.tools import Units_Encoder, WhisperLargeV3
    dims = ModelDimensions(**dict(arch.WHISPER_LARGE_V3_DIMS, n_mels=80, n_audio_state=256, n_audio_head=4, n_audio_layer=2))
    ue = Units_Encoder("whisper_large_v3", device="cuda", model=WhisperLargeV3.synthetic(dims, seed=0, device="cuda"))
    rng = np.random.default_rng(0)
    audio = dev((0.1 * rng.standard_normal((2, 16000))).astype(np.float32))
    units = ue.encode(audio[0], 16000)
    scale = np.exp2(rng.integers(-2, 3, units[::3].shape[0])).astype(np.float32)[:, None]
    model = types.SimpleNamespace(cluster_centers_=(units[::3].cpu().numpy() + 0.01 * rng.standard_normal((units[::3].shape)).astype(np.float32)) * scale)
    Cd = dev(model.cluster_centers_.astype(np.float32))
    want = native.kmeans_assign(units.contiguous(), Cd, native.kmeans_prepare(Cd, "cosine"), metric="cosine")
    assert torch.equal(ue.encode_tokens(audio[0], 16000, model, metric="cosine"), want)
    assert not torch.equal(ue.encode_tokens(audio[0], 16000, model), want)
    tok, nf = ue.encode_tokens_ragged(audio, [16000, 8000], model, pad_id=999, metric="cosine")
    assert torch.equal(tok[0, : nf[0]], want) and (tok[1, nf[1]:] == 999).all() and (tok[1, : nf[1]] < 999).all()
