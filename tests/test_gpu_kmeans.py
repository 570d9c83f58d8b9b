"""The k-means semantic tokenizer on a real MI355X (csrc/kmeans.hip through lds.native and the cluster / KMeansGPU surface): assignment
against float64 under an a-priori bound and against the reference's labels (tests/golden/kmeans.npz, make_kmeans_fixtures.py), ties,
bit-for-bit invariances, the Lloyd step and the fit against the reference's trajectory, k-means++ seeding, the Python surface and tools."""
import os
import subprocess
import sys

import numpy as np
import pytest

import kmeans_numpy as KN
from conftest import ROOT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOL = 2e-5      # the project's per-kernel tolerance (relative to the abs-max of the compared tensor)
CASES = ("blobs_4096x1280", "blobs_1000x256", "normal_4096x1280", "odd_333x136", "ragged_1000x256")      # make_kmeans_fixtures.CASES
FIT = dict(K=64, D=96, N=6000, seed=7, tol=1e-2, max_iter=200)                                            # make_kmeans_fixtures.FIT
SEED = dict(K=16, D=32, N=512)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def assign(X, C, **kw):
    from lds import native
    Cd = dev(C)
    return native.kmeans_assign(dev(X), Cd, native.kmeans_prepare(Cd), **kw)


@pytest.fixture(scope="module")
def fx(golden):
    return golden("kmeans.npz")


def case_inputs(fx, name):
    K, D, N, B = (int(v) for v in fx[name + ".shape"])
    sp = float(fx[name + ".spread"])
    C, X, _ = KN.make_blobs(int(fx[name + ".seed"]), K, D, N, None if sp < 0 else sp)
    return C, X, B


@pytest.mark.parametrize("name", CASES)
def test_assign_criterion(fx, name, record_margin):
    """Criterion: for every row, with distances recomputed in float64, d(x, c_label) - min_k d(x, c_k) <= eps(n),
    eps(n) = 4 (D + 2) 2^-24 |x_n| max_k |c_k| + 4 2^-24 max_k |c_k|^2.
    Derivation: d = |x|^2 - 2 s with s = x.c - |c|^2 / 2, so the arg-max of s is the arg-min of d.  An fp32 dot product of length D is off
    by at most gamma_D |x| |c|, gamma_D ~ D 2^-24 (any summation order); h = |c|^2 / 2 carries the same relative error on |c|^2 / 2 and the
    subtraction s = acc - h adds two roundings of magnitudes <= |x||c| + |c|^2 / 2: together <= (D + 2) 2^-24 |x| |c| + 2^-24 |c|^2 per score
    (second-order terms dropped).  The kernel prefers a over the true best b only if s~_a >= s~_b, i.e. s_b - s_a <= the two scores' errors,
    and d_a - d_b = 2 (s_b - s_a): two candidates, factor 2 -> the 4 in both terms.  An a-priori bound, not a tuned number.
    Consequence asserted on the "clear" fixtures (every row's float64 gap exceeds eps): EVERY label equals the reference's."""
    C, X, B = case_inputs(fx, name)
    if B:      # the ragged form: [B, T, D], rows beyond a clip's length poisoned, the pad id written there
        T, lens = X.shape[0] // B, fx[name + ".lengths"]
        Xr = X.reshape(B, T, -1).copy()
        valid = np.arange(T)[None, :] < lens[:, None]
        Xr[~valid] = np.nan
        got = assign(Xr, C, lengths=lens, pad_id=-7).cpu().numpy()
        assert (got[~valid] == -7).all()
        keep = valid.reshape(-1)
        got = np.where(keep, got.reshape(-1), fx[name + ".f64"])      # (padded rows: compared as if right)
    else:
        got = assign(X, C).cpu().numpy()
    exc, eps = KN.excess64(X, C, got), KN.eps_bound(X, C)
    worst = float((exc / eps).max())
    clear = fx[name + ".gap"] > eps
    print(f"{name}: worst excess / eps {worst:.3g}, labels differing from float64: {int((got != fx[name + '.f64']).sum())} of {len(got)}; rows whose "
          f"runner-up lies inside eps (held to the criterion only, not to label equality): {int((~clear).sum())}")
    record_margin(worst, 1.0)
    if int(fx[name + ".clear"]):
        assert clear.all()
    assert np.array_equal(got[clear], fx[name + ".sk"][clear]) and np.array_equal(got[clear], fx[name + ".f64"][clear])


def test_assign_near_ties(record_margin):
    """points on the bisector of two centres, moved off it by 0.25 / 1 / 4 x eps (in squared distance): labels may legitimately differ inside
    eps (the criterion still holds); rows whose float64 gap exceeds eps must get the float64 label"""
    rng = np.random.default_rng(5)
    K, D, n = 200, 64, 300      # two centre blocks
    C = (rng.standard_normal((K, D)) * 4).astype(np.float32)
    c0, c1 = C[3].astype(np.float64), C[150].astype(np.float64)
    u = (c1 - c0) / np.linalg.norm(c1 - c0)
    w = rng.standard_normal((3 * n, D)) * 0.3
    w -= (w @ u)[:, None] * u[None, :]
    base = (c0 + c1) / 2 + w
    eps0 = KN.eps_bound(base, C)
    f = np.repeat([0.25, 1.0, 4.0], n) * rng.choice([-1.0, 1.0], 3 * n)
    X = (base + (f * eps0 / (2 * np.linalg.norm(c1 - c0)))[:, None] * u[None, :]).astype(np.float32)
    got = assign(X, C).cpu().numpy()
    lab, gap = KN.assign64(X, C)
    eps = KN.eps_bound(X, C)
    assert set(np.unique(lab)) <= {3, 150}
    worst = float((KN.excess64(X, C, got) / eps).max())
    print(f"near ties: worst excess / eps {worst:.3g}; rows inside eps {int((gap <= eps).sum())}, of them labelled unlike float64 "
          f"{int((got != lab)[gap <= eps].sum())}")
    record_margin(worst, 1.0)
    assert (gap > eps).sum() >= n // 2 and np.array_equal(got[gap > eps], lab[gap > eps])


@pytest.mark.parametrize("N", [7, 70000])      # centre blocks split over workgroups / walked by one workgroup
def test_ties_lowest_index(N):
    rng = np.random.default_rng(9)
    K, D = 300, 64
    C = rng.standard_normal((K, D)).astype(np.float32)
    C[200], C[290], C[140], C[299] = C[5], C[5], C[130], C[130]      # copies at higher indices, in other centre blocks
    src = np.where(np.arange(N) % 2 == 0, 5, 130)
    X = (C[src] + 0.01 * rng.standard_normal((N, D))).astype(np.float32)
    X[:2] = C[[5, 130]]      # and the centres themselves
    got = assign(X, C).cpu().numpy()
    assert np.array_equal(got, src)


def test_assign_invariances():
    """bit for bit: repeats; a row alone and inside N = 3, 1500, 12,000 at other positions; NaN / Inf / 1e30 in OTHER rows; a poisoned workspace"""
    from lds import native
    C, X, _ = KN.make_blobs(21, 1000, 256, 12000, 0.5)
    Cd, Xd = dev(C), dev(X)
    h = native.kmeans_prepare(Cd)
    lab, best = native.kmeans_assign(Xd, Cd, h, return_best=True)
    for _ in range(5):
        l2, b2 = native.kmeans_assign(Xd, Cd, h, return_best=True)
        assert torch.equal(l2, lab) and torch.equal(b2.view(torch.int32), best.view(torch.int32))
    rows = [0, 127, 128, 1499, 6001, 11999]
    for r in rows:
        l1, b1 = native.kmeans_assign(Xd[r:r + 1].contiguous(), Cd, h, return_best=True)
        assert l1[0] == lab[r] and b1.view(torch.int32)[0] == best.view(torch.int32)[r], r
    for n, at in ((3, 2), (1500, 777), (1500, 0), (12000, 5)):
        Y = Xd[torch.randperm(12000, generator=torch.Generator().manual_seed(n)).cuda()[:n]].contiguous()
        Y[at] = Xd[6001]
        l1, b1 = native.kmeans_assign(Y, Cd, h, return_best=True)
        assert l1[at] == lab[6001] and b1.view(torch.int32)[at] == best.view(torch.int32)[6001], (n, at)
    for poison in (float("nan"), float("inf"), -float("inf"), 1e30):
        Y = Xd.clone()
        mask = torch.ones(12000, dtype=torch.bool, device="cuda")
        mask[rows] = False
        Y[mask] = poison
        ws = torch.empty(native.kmeans_workspace_bytes(12000, 1000, 256), dtype=torch.uint8, device="cuda")
        native.debug_fill(ws[: ws.numel() // 4 * 4], 0x7FC00000 if poison != 1e30 else 0x7149F2CA)
        l1, b1 = native.kmeans_assign(Y, Cd, h, return_best=True, ws=ws)
        assert torch.equal(l1[rows], lab[rows]) and torch.equal(b1.view(torch.int32)[rows], best.view(torch.int32)[rows]), poison


@pytest.mark.parametrize("N,K", [(1, 1), (37, 100), (1501, 4097), (1, 4097), (1501, 1)])
def test_assign_odd_shapes(N, K, record_margin):
    C, X, _ = KN.make_blobs(31, K, 72, N, 0.5)      # D = 72: a partial last K-step
    got = assign(X, C).cpu().numpy()
    assert got.min() >= 0 and got.max() < K
    worst = float((KN.excess64(X, C, got) / KN.eps_bound(X, C)).max())
    record_margin(worst, 1.0)
    lab, gap = KN.assign64(X, C)
    assert np.array_equal(got[gap > KN.eps_bound(X, C)], lab[gap > KN.eps_bound(X, C)])


def _sk_model(C):
    """a scikit-learn KMeans poured from a checkpoint dict, as cluster.get_cluster_model does"""
    from sklearn.cluster import KMeans
    km = KMeans(C.shape[1])
    km.__dict__.update(n_features_in_=C.shape[1], _n_threads=4, cluster_centers_=C)
    return km


def test_assign_full_width(record_margin):
    """K 4096 x D 1280 x N 12,000 (a preprocessing batch: 8 clips of 30 s), half blob points, half pure N(0,1), against float64"""
    C, Xb, _ = KN.make_blobs(41, 4096, 1280, 6000, 0.5)
    X = np.concatenate([Xb, np.random.default_rng(42).standard_normal((6000, 1280)).astype(np.float32)])
    from lds import native
    Cd = dev(C)
    lab, best = native.kmeans_assign(dev(X), Cd, native.kmeans_prepare(Cd), return_best=True)
    got = lab.cpu().numpy()
    exc, eps = KN.excess64(X, C, got), KN.eps_bound(X, C)
    worst = float((exc / eps).max())
    # the reference's euc_sim in fp32 (kmeans.py:115) on the same rows: its own excess under the same measure
    Xt, Ct = torch.from_numpy(X), torch.from_numpy(C)
    ref = (2 * Xt @ Ct.T - (Xt ** 2).sum(1)[:, None] - (Ct ** 2).sum(1)[None, :]).max(-1)[1].numpy()
    worst_ref = float((KN.excess64(X, C, ref) / eps).max())
    # scikit-learn's predict (the reference's get_cluster_result) on the same rows
    import cluster
    sk = cluster.get_cluster_result(_sk_model(C), X)
    worst_sk = float((KN.excess64(X, C, sk) / eps).max())
    l64, gap = KN.assign64(X, C)
    print(f"full width: worst excess / eps native {worst:.3g}, reference euc_sim fp32 (CPU) {worst_ref:.3g}, scikit-learn {worst_sk:.3g}; labels unlike "
          f"float64: native {int((got != l64).sum())}, reference {int((ref != l64).sum())}, scikit-learn {int((sk != l64).sum())} of {len(got)}; "
          f"rows inside eps {int((gap <= eps).sum())}")
    record_margin(worst, 1.0)
    record_margin(worst_ref, 1.0, "reference_euc_sim_fp32")      # the reference's own results under the same criterion, on the record
    record_margin(worst_sk, 1.0, "scikit_learn")
    assert np.array_equal(got[gap > eps], l64[gap > eps])
    # the winning score: |x|^2 - 2 best = the squared distance to the chosen centre
    d = (X.astype(np.float64) ** 2).sum(1) - 2 * best.cpu().numpy().astype(np.float64)
    true = ((X.astype(np.float64) - C[got].astype(np.float64)) ** 2).sum(1)
    assert np.abs(d - true).max() <= eps.max()


# ---- the Lloyd step and the fit ----
def fit_inputs(fx):
    return KN.make_blobs(FIT["seed"], FIT["K"], FIT["D"], FIT["N"], 0.5)[1]


def test_update_step_vs_fixture(fx, record_margin):
    """every iteration of the reference's run on its own: the float64 state in, the fixture's labels given, the new state compared"""
    from lds import native
    X = fit_inputs(fx)
    Xd = dev(X)
    C64, np64 = fx["fit.start"].astype(np.float64), np.ones(FIT["K"])
    Cx, npx = C64, np64      # the unrounded float64 chain (the fixture's float64 run)
    worst_c = worst_n = worst_e = 0.0
    for i, lab in enumerate(fx["fit.labels"].astype(np.int64)):
        Cd, npd = dev(C64.astype(np.float32)), dev(np64.astype(np.float32))
        h = native.kmeans_prepare(Cd)
        err = native.kmeans_update(Xd, dev(lab), Cd, h, npd)
        C64n, np64n, e64, _ = KN.lloyd_step64(X, lab, C64.astype(np.float32), np64.astype(np.float32))
        worst_c = max(worst_c, float(np.abs(Cd.cpu().numpy() - C64n).max() / np.abs(C64n).max()))
        worst_n = max(worst_n, float(np.abs(npd.cpu().numpy() - np64n).max() / np.abs(np64n).max()))
        worst_e = max(worst_e, abs(float(err) - e64) / e64)
        assert torch.equal(h.view(torch.int32), native.kmeans_prepare(Cd).view(torch.int32))      # h refreshed
        C64, np64 = C64n, np64n
        Cx, npx = KN.lloyd_step64(X, lab, Cx, npx)[:2]
    print(f"update: centroids {worst_c:.2e}, num_points {worst_n:.2e} of abs-max, error {worst_e:.2e} relative "
          f"(the reference's own fp32-vs-float64 gap on the final centroids: {float(fx['fit.gap']):.2e})")
    record_margin(worst_c, TOL, "centroids")
    record_margin(worst_n, TOL, "num_points")
    record_margin(worst_e, TOL, "error")
    assert np.abs(Cx - fx["fit.centroids64"]).max() < 1e-9      # (the chain of float64 steps is the fixture's float64 run)


def test_update_empty_cluster_and_repeat(fx):
    from lds import native
    X = fit_inputs(fx)
    Xd = dev(X)
    lab = fx["fit.labels"][0].astype(np.int64)
    lab[lab == 3] = 4      # cluster 3 is empty
    res = []
    for poison in (None, 0x7FC00000, 0xFFFFFFFF):
        Cd, npd = dev(fx["fit.start"]), torch.ones(FIT["K"], device="cuda")
        h = native.kmeans_prepare(Cd)
        ws = torch.empty(native.kmeans_workspace_bytes(FIT["N"], FIT["K"], FIT["D"]), dtype=torch.uint8, device="cuda")
        if poison is not None:
            native.debug_fill(ws[: ws.numel() // 4 * 4], poison)
        err = native.kmeans_update(Xd, dev(lab), Cd, h, npd, ws=ws)
        res.append((Cd, npd, h, err.reshape(1)))
    assert (res[0][0][3] == 0).all() and res[0][1][3] == 1      # lr = 1 on the first step: the zero c_grad row itself
    for r in res[1:]:
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(r, res[0]))


def test_fit_from_captured_start(fx, record_margin):
    from cluster.kmeans import KMeansGPU
    X = fit_inputs(fx)
    km = KMeansGPU(FIT["K"], max_iter=FIT["max_iter"], tol=FIT["tol"], init=fx["fit.start"], minibatch=10 ** 9)
    last = km.fit_predict(torch.from_numpy(X))
    assert km.n_iter_ == len(fx["fit.errors"]), (km.n_iter_, len(fx["fit.errors"]))
    assert last.dtype == torch.int64 and last.is_cuda and np.array_equal(last.cpu().numpy(), fx["fit.labels"][-1].astype(np.int64))
    e = np.abs(np.array(km.errors_) - fx["fit.errors64"]) / fx["fit.errors64"]
    print(f"fit: {km.n_iter_} iterations, worst error-trajectory deviation {e.max():.2e}")
    record_margin(float(np.abs(km.centroids.cpu().numpy() - fx["fit.centroids64"]).max() / np.abs(fx["fit.centroids64"]).max()), TOL)


def test_fit_minibatch_mode(fx, record_margin):
    """minibatch < N // 2: a fresh torch.randint subset per iteration; the float64 restatement replays the same draws"""
    from cluster.kmeans import KMeansGPU
    X = fit_inputs(fx)
    km = KMeansGPU(FIT["K"], max_iter=12, tol=0.0, init=fx["fit.start"], minibatch=1000)
    torch.manual_seed(123)
    last = km.fit_predict(torch.from_numpy(X))
    torch.manual_seed(123)
    ref = KN.fit64(X, fx["fit.start"], 12, 0.0, batches=lambda i: torch.randint(0, FIT["N"], [1000]).numpy())
    assert km.n_iter_ == 12 and np.array_equal(last.cpu().numpy(), ref["labels"][-1])
    record_margin(float(np.abs(km.centroids.cpu().numpy() - ref["centroids"]).max() / np.abs(ref["centroids"]).max()), TOL)


# ---- seeding ----
def test_seeding_fixture(fx):
    from lds import native
    X = KN.make_blobs(int(fx["seed.seed"]), SEED["K"], SEED["D"], SEED["N"], 0.5)[1]
    for _ in range(2):
        C, picked = native.kmeans_seed(dev(X), SEED["K"], int(fx["seed.first"]), dev(fx["seed.uniforms"]))
        assert np.array_equal(picked.cpu().numpy(), fx["seed.picks"])
        assert np.array_equal(C.cpu().numpy(), X[fx["seed.picks"]])


def test_seeding_large_every_pick(record_margin):
    """K 256, N 20,000, D 128: pick sequences are chaotic, so every pick is verified on its own: the float64 CDF rebuilt from the NATIVE picks
    so far must contain the draw in the picked point's interval widened by 2 (D + 2) 2^-24 on each side (the fp32 distances' relative error
    bound on numerator and denominator; the prefix itself is accumulated in double)"""
    from lds import native
    K, N, D = 256, 20000, 128
    X = KN.make_blobs(77, 64, D, N, 0.5)[1]
    u = np.random.default_rng(78).random(K - 1).astype(np.float32)
    C, picked = native.kmeans_seed(dev(X), K, 4321, dev(u))
    picked = picked.cpu().numpy()
    assert picked[0] == 4321 and np.array_equal(C.cpu().numpy(), X[picked])
    widen = 2 * (D + 2) * 2.0 ** -24
    X64 = X.astype(np.float64)
    mind, worst = np.full(N, np.inf), 0.0
    for i in range(1, K):
        mind = np.minimum(mind, np.sqrt(((X64 - X64[picked[i - 1]]) ** 2).sum(1)))
        cum = np.cumsum(mind / mind.sum())
        j, ui = int(picked[i]), float(u[i - 1])
        lo = cum[j - 1] if j else 0.0
        # how far outside [lo, cum[j]] the draw lies, in units of the allowed widening
        worst = max(worst, max(lo - ui, ui - cum[j], 0.0) / widen)
    print(f"seeding: worst distance of a draw outside its pick's interval {worst:.3g} x the allowed widening")
    record_margin(worst, 1.0)


# ---- the surface ----
def test_fit_predict_recovers_planted_partition():
    from cluster.kmeans import KMeansGPU
    rng = np.random.default_rng(3)
    K, D, N = 8, 64, 4000
    cent = (rng.standard_normal((K, D)) * 10).astype(np.float32)
    planted = rng.integers(0, K, N)
    X = (cent[planted] + 0.01 * rng.standard_normal((N, D))).astype(np.float32)
    torch.manual_seed(0)
    km = KMeansGPU(K, max_iter=50, tol=1e-6)
    lab = km.fit_predict(torch.from_numpy(X)).cpu().numpy()
    table = {}
    for a, b in zip(lab, planted):
        assert table.setdefault(int(a), int(b)) == int(b)
    assert len(set(table.values())) == K
    v, i = km.max_sim(torch.from_numpy(X[:100]), km.centroids)
    d = ((X[:100].astype(np.float64)[:, None] - km.centroids.cpu().numpy().astype(np.float64)[None]) ** 2).sum(-1)
    assert np.array_equal(i.cpu().numpy(), d.argmin(1)) and np.abs(-v.cpu().numpy() - d.min(1)).max() < 1e-2


def test_max_sim_many_rows():
    """max_sim is the reference class's way to label new data: more rows than the codebook limit of 65,536"""
    from cluster.kmeans import KMeansGPU
    C, X, _ = KN.make_blobs(19, 50, 32, 70001, 0.5)
    v, i = KMeansGPU(50).max_sim(torch.from_numpy(X), torch.from_numpy(C))
    lab, gap = KN.assign64(X, C)
    keep = gap > KN.eps_bound(X, C)
    assert keep.mean() > 0.99 and np.array_equal(i.cpu().numpy()[keep], lab[keep])
    d = ((X.astype(np.float64) - C[lab].astype(np.float64)) ** 2).sum(1)
    assert v.shape == (70001,) and np.abs(-v.cpu().numpy() - d).max() < 1e-3 * d.max()


def test_train_cluster_roundtrip(tmp_path):
    import cluster
    C0, X, _ = KN.make_blobs(13, 32, 64, 3000, 0.3)
    torch.manual_seed(1)
    ck = cluster.train_cluster(X, 32, max_iter=30, tol=1e-4)
    assert sorted(ck) == ["_n_threads", "cluster_centers_", "n_features_in_"] and ck["cluster_centers_"].shape == (32, 64)
    torch.save(ck, tmp_path / "semantic_codebook.pt")
    model = cluster.get_cluster_model(str(tmp_path / "semantic_codebook.pt"))
    units = dev(X[:500])
    got = cluster.get_cluster_result(model, units)
    assert got.is_cuda and got.dtype == torch.int64
    assert np.array_equal(got.cpu().numpy(), cluster.get_cluster_result(model, units.cpu().numpy()))
    got3 = cluster.get_cluster_result(model, units.reshape(5, 100, 64))
    assert torch.equal(got3.reshape(-1), got)
    cen = cluster.get_cluster_center_result(model, units)
    assert np.array_equal(cen.cpu().numpy(), model.cluster_centers_[got.cpu().numpy()].astype(np.float32))


def test_encode_tokens_equals_encode_then_assign():
    import types

    from encoder.whisper.model import ModelDimensions
    from lds import arch, native
    from tools.tools import Units_Encoder, WhisperLargeV3
    dims = ModelDimensions(**dict(arch.WHISPER_LARGE_V3_DIMS, n_mels=80, n_audio_state=256, n_audio_head=4, n_audio_layer=2))
    ue = Units_Encoder("whisper_large_v3", device="cuda", model=WhisperLargeV3.synthetic(dims, seed=0, device="cuda"))
    rng = np.random.default_rng(0)
    audio = dev((0.1 * rng.standard_normal((2, 16000))).astype(np.float32))
    units = ue.encode(audio[0], 16000)
    model = types.SimpleNamespace(cluster_centers_=units[::3].cpu().numpy() + 0.01 * rng.standard_normal((units[::3].shape)).astype(np.float32))
    Cd = dev(model.cluster_centers_.astype(np.float32))
    want = native.kmeans_assign(units.contiguous(), Cd, native.kmeans_prepare(Cd))
    assert torch.equal(ue.encode_tokens(audio[0], 16000, model), want)
    tok, nf = ue.encode_tokens_ragged(audio, [16000, 8000], model, pad_id=999)
    assert torch.equal(tok[0, : nf[0]], want) and (tok[1, nf[1]:] == 999).all() and (tok[1, : nf[1]] < 999).all()
    assert torch.equal(tok[1, : nf[1]], ue.encode_tokens(audio[1, :8000], 16000, model))


def test_tools_train_codebook_and_extract_tokens(tmp_path):
    import cluster
    C0, X, _ = KN.make_blobs(17, 16, 64, 1200, 0.3)
    udir = tmp_path / "units"
    udir.mkdir()
    cuts = [0, 100, 333, 700, 1200]
    for i in range(4):
        np.save(udir / f"clip{i}.npy", X[cuts[i]:cuts[i + 1]])
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    ck = tmp_path / "semantic_codebook.pt"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_codebook.py"), str(udir), "--out", str(ck), "--n_clusters", "16",
                        "--max_iter", "20"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    model = cluster.get_cluster_model(str(ck))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "extract_tokens.py"), str(udir), "--codebook", str(ck), "--batch", "3"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    for i in range(4):
        tok = np.load(tmp_path / "semantic_token" / f"clip{i}.npy")
        assert tok.dtype == np.int64 and np.array_equal(tok, model.predict(X[cuts[i]:cuts[i + 1]]))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "extract_tokens.py"), str(udir), "--synthetic", "100", "--out", str(tmp_path / "syn")],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    Cs = np.random.default_rng(0).standard_normal((100, 64)).astype(np.float32)
    assert np.array_equal(np.load(tmp_path / "syn" / "clip2.npy"), KN.assign64(X[333:700], Cs)[0])


def test_tool_extract_tokens_from_audio(tmp_path):
    """16 kHz clips -> tokens in one tool = tools/extract_units.py followed by the unit-file form, with the same seeded encoder and centres"""
    rng = np.random.default_rng(2)
    cdir = tmp_path / "clips"
    cdir.mkdir()
    for i, n in enumerate((16000, 9000, 300)):      # (the last one is shorter than 400 samples: padded as encode does)
        np.save(cdir / f"clip{i}.npy", (0.1 * rng.standard_normal(n)).astype(np.float32))
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    run = lambda *argv: subprocess.run([sys.executable] + [str(x) for x in argv], env=env, capture_output=True, text=True, timeout=900)      # noqa: E731
    r = run(os.path.join(ROOT, "tools", "extract_tokens.py"), cdir, "--from-audio", "--synthetic-encoder", "--layers", "2", "--synthetic", "64",
            "--out", tmp_path / "tok_audio", "--batch", "2")
    assert r.returncode == 0, r.stderr[-2000:]
    r = run(os.path.join(ROOT, "tools", "extract_units.py"), cdir, "--out", tmp_path / "units", "--synthetic", "--layers", "2", "--batch", "2")
    assert r.returncode == 0, r.stderr[-2000:]
    r = run(os.path.join(ROOT, "tools", "extract_tokens.py"), tmp_path / "units", "--synthetic", "64", "--out", tmp_path / "tok_units")
    assert r.returncode == 0, r.stderr[-2000:]
    for i in range(3):
        a, b = np.load(tmp_path / "tok_audio" / f"clip{i}.npy"), np.load(tmp_path / "tok_units" / f"clip{i}.npy")
        assert a.dtype == np.int64 and a.ndim == 1 and len(a) > 0 and a.min() >= 0 and a.max() < 64 and np.array_equal(a, b)
