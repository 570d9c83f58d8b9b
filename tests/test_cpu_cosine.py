"""The cosine metric without a GPU: the float64 oracle (tests/cosine_numpy.py) against the fixture recorded from the reference's
KMeansGPU(mode="cosine") -- KMeansCosineGPU here -- (tests/golden/kmeans_cosine.npz), what fp32 arithmetic makes of the definitions (exact on the lattice, inside the
a-priori bounds on Gaussian inputs), the Python surface's refusals and the index file's "metric" key, and the new C entries in the binding."""
import os
import re

import numpy as np
import pytest

import cosine_numpy as CN
import kmeans_numpy as KM
import knn_numpy as KN
from conftest import ROOT

f32 = np.float32


@pytest.fixture(scope="module")
def fx(golden):
    return golden("kmeans_cosine.npz")


# ---- the oracle against the reference ----
@pytest.mark.parametrize("name", list(CN.BLOBS))
def test_oracle_labels_equal_the_references(fx, name):
    K, D, N, _, B, lens = CN.BLOBS[name]
    assert tuple(fx[f"{name}.shape"]) == (K, D, N, B)
    C, X, _ = CN.scaled_blobs(int(fx[f"{name}.seed"]), K, D, N)
    lab, best, gap = CN.assign64(X, C)
    assert np.array_equal(lab, fx[f"{name}.ref"]) and np.array_equal(lab, fx[f"{name}.f64"])
    # (float64 matrix products differ in their last bits between BLAS builds and thread counts: the recorded gaps are compared to 1e-9)
    assert np.allclose(gap, fx[f"{name}.gap"], rtol=1e-9, atol=1e-12) and gap.min() > CN.search_bound(D)      # "clear": no row within the bound of a tie
    assert np.abs(fx[f"{name}.ref_sim"] - best).max() <= CN.sim_bound(D)
    # the scaling moves Euclidean labels and leaves cosine ones alone: a Euclidean kernel passed off as cosine fails these cases
    euc = KM.assign64(X, C)[0]
    assert int((euc != lab).sum()) == int(fx[f"{name}.euclidean_differs"]) >= N // 5
    C0, X0, _ = KM.make_blobs(int(fx[f"{name}.seed"]), K, D, N)
    assert np.array_equal(CN.assign64(X0, C0)[0], lab)
    if lens is not None:
        assert list(fx[f"{name}.lengths"]) == list(lens) and max(lens) <= N // B


def test_oracle_fit_follows_the_reference_iteration_by_iteration(fx):
    F = CN.FIT
    _, X, _ = CN.scaled_blobs(F["seed"], F["K"], F["D"], F["N"])
    got = CN.fit64(X, fx["fit.start"], F["max_iter"], F["tol"])
    ref_labels = fx["fit.labels"]
    assert got["n_iter"] == len(ref_labels) == len(fx["fit.errors"]) and 2 <= got["n_iter"] < F["max_iter"]
    for i, lab in enumerate(got["labels"]):
        assert np.array_equal(lab, ref_labels[i]), i
    assert np.allclose(got["errors"], fx["fit.errors64"], rtol=1e-9, atol=0)
    assert np.allclose(got["errors"], fx["fit.errors"], rtol=1e-4, atol=0)      # the reference's fp32 sums of 6144 squares
    assert np.abs(got["centroids"] - fx["fit.centroids"]).max() <= 1e-6 * np.abs(got["centroids"]).max()
    assert got["errors"][-1] <= F["tol"] < got["errors"][-2]


# ---- what fp32 arithmetic makes of the definitions ----
@pytest.mark.parametrize("case", CN.LATTICE, ids=lambda c: "x".join(map(str, c)))
def test_lattice_is_exact_in_fp32(case):
    N, M, D, k = case
    X, P = CN.lattice_case(N, M, D)
    n2 = (P.astype(np.float64) ** 2).sum(1)
    assert set(np.unique(n2)) <= {1.0, 4.0, 16.0, 64.0, 256.0, 1024.0}
    r32 = CN.row_const(P, f32)
    assert r32.dtype == f32 and np.array_equal(r32.astype(np.float64), CN.row_const(P)) and set(np.unique(r32)) <= {2.0 ** -e for e in range(6)}
    s32, s64 = CN.scores(X, P, f32), CN.scores(X, P)
    assert s32.dtype == f32 and np.array_equal(s32.astype(np.float64), s64)
    assert np.array_equal(CN.sims(X, P, f32).astype(np.float64), CN.sims(X, P))
    idx, sim = CN.search64(X, P, k)
    assert np.array_equal(KN.topk_stable(s32, k), idx)
    ties = int((np.diff(np.take_along_axis(s64, idx, 1), axis=1) == 0).sum())      # exactly equal scores inside the top k: the index decides
    assert ties >= N // 2, ties
    assert (np.diff(idx, axis=1)[np.diff(np.take_along_axis(s64, idx, 1), axis=1) == 0] > 0).all()


def test_row_constant_definition():
    v = np.zeros((5, 8), f32)
    v[1, 0], v[2, :4], v[3, :4], v[4, 0] = 2.0, 2.0, 4.0, 1e-20
    r = CN.row_const(v, f32)
    assert list(r[:4]) == [f32(1e12), 0.5, 0.25, 0.125] and r[4] == f32(1e12)      # the eps of F.normalize; powers of two exactly
    assert np.array_equal(CN.scores(v, v, f32)[0], np.zeros(5, f32)) and not np.isnan(CN.sims(v, v, f32)).any()


def test_bounds_hold_for_fp32_numpy():
    N, M, D, k = CN.GAUSSIAN[0]
    X, P = CN.gaussian_case(N, M, D)
    want, sim_want = CN.search64(X, P, k)
    s32 = CN.scores(X, P, f32)
    idx = KN.topk_stable(s32, k)
    got_sim = (np.take_along_axis(s32, idx, 1) * CN.row_const(X, f32)[:, None]).astype(f32)
    true = CN.sim64(X, P, idx)
    assert np.abs(got_sim - true).max() <= CN.sim_bound(D)
    assert (sim_want - true).max() <= CN.search_bound(D) and (true - sim_want).max() <= 1e-15
    # distances and both weightings, fp32 evaluation on its own neighbours
    a = (X * CN.row_const(X, f32)[:, None]).astype(f32)
    b = (P[idx] * CN.row_const(P, f32)[idx][:, :, None]).astype(f32)
    d32 = np.maximum(f32(0.5) * ((a[:, None, :] - b) ** 2).sum(2, dtype=f32), f32(CN.FLOOR))
    for how in ("inverse_square", "uniform"):
        y64, d64, _ = CN.blend64(X, P, idx, 0.5, how)
        assert (np.abs(d32 - d64) <= CN.dist_bound(D, d64) * d64).all()
        w32 = CN.weights64(d32.astype(np.float64), idx >= 0, how).astype(f32)
        y32 = (f32(0.5) * X + f32(0.5) * np.einsum("nk,nkd->nd", w32, P[idx]).astype(f32)).astype(f32)
        assert np.abs(y32 - y64).max() <= CN.blend_bound(X, P, d64.min())
    # Euclidean distances with uniform weights: knn_numpy's bound as it is
    i2 = KN.search64(X, P, k)[0]
    y64 = CN.blend64(X, P, i2, 0.5, "uniform", metric="l2")[0]
    y32 = (f32(0.5) * X + f32(0.5) * P[i2].mean(1, dtype=f32)).astype(f32)
    assert np.abs(y32 - y64).max() <= KN.blend_bound(X, P)


def test_uniform_weights_are_over_the_rows_found():
    X, P = CN.lattice_case(4, 16, 8)
    idx = np.array([[3, 5, -1, -1], [1, -1, -1, -1], [-1, -1, -1, -1], [0, 1, 2, 3]])
    y, d, w = CN.blend64(X, P, idx, 1.0, "uniform")
    assert np.array_equal(w[0], [0.5, 0.5, 0, 0]) and np.array_equal(w[1], [1, 0, 0, 0]) and not w[2].any() and np.array_equal(w[3], [0.25] * 4)
    assert np.array_equal(y[1], P[1]) and np.array_equal(y[0], 0.5 * (P[3].astype(np.float64) + P[5])) and not d[2].any()


# ---- the Python surface ----
def test_bad_metric_weights_and_mode_raise_before_any_device():
    import types

    import torch

    import cluster
    from cluster.index import UnitsIndex
    from cluster.kmeans import KMeansCosineGPU, KMeansGPU
    from lds import native
    pool = np.zeros((16, 8), f32)
    for bad in ("euclidean", "COSINE", None, 1):
        with pytest.raises(ValueError, match="metric"):
            UnitsIndex(pool, metric=bad)
        with pytest.raises(ValueError, match="metric"):
            native.metric_code(bad)
    x = torch.zeros(4, 8)      # a CPU tensor: the device path would refuse it with a RuntimeError -- the ValueError comes first
    for ix in (UnitsIndex(pool), UnitsIndex(pool, metric="cosine")):
        for bad in ("mean", "inverse", None, 0):
            with pytest.raises(ValueError, match="weights"):
                ix.retrieve(x, k=2, weights=bad)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ix.retrieve(x, k=2, weights="uniform")
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ix.search(x, k=2)
    c, h = torch.zeros(2, 8), torch.zeros(2)
    for call in (lambda: native.kmeans_prepare(c, "cos"), lambda: native.kmeans_assign(x, c, h, metric="cos"),
                 lambda: native.kmeans_update(x, torch.zeros(4, dtype=torch.int64), c, h, torch.ones(2), metric="cos"),
                 lambda: native.knn_prepare(c, "cos"), lambda: native.knn_search(x, c, h, 1, metric="cos"),
                 lambda: native.knn_retrieve(x, c, h, 1, 0.5, metric="cos"), lambda: native.knn_retrieve(x, c, h, 1, 0.5, weights="mean"),
                 lambda: native.ivf_search(x, c, h, 1, None, 1, metric="cos"), lambda: native.ivf_retrieve(x, c, h, 1, 0.5, None, 1, weights="mean")):
        with pytest.raises(ValueError, match="metric|weights"):
            call()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        native.kmeans_prepare(c, "cosine")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        native.knn_prepare(c, "cosine")
    model = types.SimpleNamespace(cluster_centers_=np.zeros((2, 8), f32))
    with pytest.raises(ValueError, match="metric"):
        cluster.get_cluster_result(model, x, metric="cos")
    with pytest.raises(ValueError, match="device path"):
        cluster.get_cluster_result(model, np.zeros((4, 8), f32), metric="cosine")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cluster.get_cluster_result(model, x, metric="cosine")
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # the refusal is the device's, not NotImplementedError
        KMeansGPU(8, mode="cosine", device=torch.device("cpu"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KMeansCosineGPU(8, device=torch.device("cpu"))
    assert issubclass(KMeansCosineGPU, KMeansGPU) and KMeansCosineGPU._metric == "cosine" and KMeansGPU._metric == "l2"
    with pytest.raises(NotImplementedError, match="never formed"):
        KMeansCosineGPU.cos_sim(x, c)
    with pytest.raises(ValueError, match="mode"):
        cluster.train_cluster(np.zeros((4, 8), f32), 2, mode="cos", device="cpu")
    from tools.tools import Units_Encoder
    ue = Units_Encoder.__new__(Units_Encoder)      # (no encoder behind it: the metric is checked before it would run)
    with pytest.raises(ValueError, match="metric"):
        ue.encode_tokens(x, 16000, model, metric="cos")
    with pytest.raises(ValueError, match="metric"):
        ue.encode_tokens_ragged(x, [4], model, pad_id=-1, metric="cos")


def test_index_file_keeps_the_metric(tmp_path):
    import torch

    from cluster.index import UnitsIndex
    pool = np.random.default_rng(0).standard_normal((40, 16)).astype(f32)
    cos = UnitsIndex(pool, metric="cosine")
    assert cos.metric == "cosine" and cos.state()["metric"] == "cosine"
    cos.save(tmp_path / "cos.pt")
    back = UnitsIndex.load(tmp_path / "cos.pt")
    assert back.metric == "cosine" and np.array_equal(back.pool, pool) and back.state()["metric"] == "cosine"
    plain = UnitsIndex(pool)
    assert plain.metric == "l2"
    plain.save(tmp_path / "l2.pt")
    assert UnitsIndex.load(tmp_path / "l2.pt").metric == "l2"
    old = {k: v for k, v in plain.state().items() if k != "metric"}      # a file from before the key existed
    torch.save(old, tmp_path / "old.pt")
    assert "metric" not in torch.load(tmp_path / "old.pt", weights_only=False) and UnitsIndex.load(tmp_path / "old.pt").metric == "l2"
    torch.save(dict(old, metric="manhattan"), tmp_path / "bad.pt")
    with pytest.raises(ValueError, match="metric"):
        UnitsIndex.load(tmp_path / "bad.pt")


def test_tools_take_the_metric_arguments():
    import infer_svc
    a = infer_svc.parse_args(["--synthetic", "--index", "x.pt", "--index_k", "4", "--index_weights", "uniform", "--index_ratio", "1.0"])
    assert a.index_weights == "uniform" and infer_svc.parse_args(["--synthetic"]).index_weights == "inverse_square"
    with pytest.raises(SystemExit):
        infer_svc.parse_args(["--synthetic", "--index_weights", "mean"])
    for tool, flag in (("train_codebook.py", "--mode"), ("extract_tokens.py", "--metric"), ("train_units_index.py", "--metric"),
                       ("bench_knn.py", "--metric"), ("bench_kmeans.py", "--metric")):
        assert f'"{flag}"' in open(os.path.join(ROOT, "tools", tool)).read(), tool
    assert '"--index_weights"' in open(os.path.join(ROOT, "infer_tts.py")).read()


# ---- the binding ----
def _header_params(name):
    """{function: [(type, parameter name)]} of include/<name>"""
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    out = {}
    for fn, params in re.findall(r"\b(lds_\w+)\s*\(([^()]*)\)\s*;", hdr):
        out[fn] = [("*" if "*" in p else [w for w in re.findall(r"\w+", p) if w != "const"][0], re.findall(r"\w+", p)[-1]) for p in params.split(",")]
    return out


def test_metric_entries_are_their_namesakes_plus_the_choice():
    """every *_metric entry is declared in the header, bound with the header's signature, and is its namesake with `int metric` (and, where a
    blend follows, `int weights` right after it) added -- so tests/test_cpu_boundary.py's signature check covers them"""
    import ctypes as C

    from lds import native
    public, test = _header_params("lds.h"), _header_params("lds_test.h")
    want = {f"lds_kmeans_{n}_metric" for n in ("prepare", "assign", "assign_ragged", "update")}
    want |= {f"lds_knn_{n}_metric" for n in ("prepare", "search", "retrieve", "retrieve_ragged")}
    want |= {f"lds_ivf_{n}_metric" for n in ("search", "retrieve", "retrieve_ragged")}
    want_test = {"lds_test_knn_search_metric", "lds_test_ivf_search_metric"}
    assert {n for n in public if n.endswith("_metric")} == want and {n for n in test if n.endswith("_metric")} == want_test
    assert want <= set(native.EXPORTS) and want_test <= set(native.TEST_EXPORTS)
    kinds = {"*": C.c_void_p, "int": C.c_int, "size_t": C.c_size_t, "float": C.c_float, "int64_t": C.c_int64}
    L = native.lib()
    for fn in sorted(want | want_test):
        params = {**public, **test}[fn]
        base = {**public, **test}[fn[: -len("_metric")]]
        names = [n for _, n in params]
        added = ["metric", "weights"] if "retrieve" in fn else ["metric"]
        at = names.index("metric")
        assert names[at:at + len(added)] == added and all(t == "int" for t, _ in params[at:at + len(added)]), fn
        assert params[:at] + params[at + len(added):] == base, fn
        assert list(getattr(L, fn).argtypes) == [kinds[t] for t, _ in params] and getattr(L, fn).restype is C.c_int, fn
    hdr = open(os.path.join(ROOT, "include", "lds.h")).read()
    assert re.search(r"#define LDS_METRIC_L2 0\b", hdr) and re.search(r"#define LDS_METRIC_COSINE 1\b", hdr)
    assert re.search(r"#define LDS_WEIGHTS_INVERSE_SQUARE 0\b", hdr) and re.search(r"#define LDS_WEIGHTS_UNIFORM 1\b", hdr)
    assert native.METRICS == {"l2": 0, "cosine": 1} and native.WEIGHTS == {"inverse_square": 0, "uniform": 1}
    assert "overflows fp32" in hdr      # the documented limit of the row constant
