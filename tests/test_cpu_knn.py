"""Units retrieval without a GPU: the float64 oracle (tests/knn_numpy.py) against scipy's k-d tree, the UnitsIndex file and its Python-layer
errors, the C entries' limits through the built library (they answer before any device work), the index tool's reduction rule, and what
fp32 arithmetic attains on the very inputs tests/test_gpu_knn.py uses."""
import ctypes as ct
import importlib.util
import os

import numpy as np
import pytest

import knn_numpy as KN
from conftest import ROOT

torch = pytest.importorskip("torch")

ENTRIES = ("lds_knn_prepare", "lds_knn_workspace_bytes", "lds_knn_search", "lds_knn_retrieve", "lds_knn_retrieve_ragged")


def test_oracle_neighbours_equal_ckdtree():
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(0)
    X, P = rng.standard_normal((60, 16)).astype(np.float32), rng.standard_normal((500, 16)).astype(np.float32)
    idx, score = KN.search64(X, P, 8)
    d_tree, i_tree = cKDTree(P.astype(np.float64)).query(X.astype(np.float64), k=8)
    assert np.array_equal(idx, i_tree)      # (continuous data: no ties, so the order is the tree's too)
    d = KN.dist64(X, P, idx)
    assert np.allclose(d, d_tree ** 2, rtol=1e-12) and (np.diff(d, axis=1) >= 0).all()
    assert np.allclose((X.astype(np.float64) ** 2).sum(1)[:, None] - 2 * score, d, atol=1e-10)


def test_oracle_tie_rule_floor_weights_and_ragged():
    X, P = KN.lattice_case(40, 30, 8)
    P3 = np.concatenate([P, P, P])      # every row three times: the copies tie exactly, the lower index first
    idx, sc = KN.search64(X, P3, 6)
    s = KN.scores(X, P3)
    assert (idx[:, 0] < 30).all() and np.array_equal(sc[:, 0], s.max(1)) and (sc[:, :3] == sc[:, :1]).all()
    assert (np.diff(sc, axis=1) <= 0).all() and (np.diff(idx, axis=1)[np.diff(sc, axis=1) == 0] > 0).all()
    assert all(np.array_equal(np.sort(s[n])[::-1][:6], sc[n]) for n in range(40))
    y, d, w = KN.blend64(P[:5], P, np.arange(5)[:, None], 1.0)      # a query that is a pool row: d = 0 takes the floor
    assert (d == KN.FLOOR).all() and (w == 1).all() and np.array_equal(y, P[:5].astype(np.float64))
    y, d, w = KN.blend64(X, P, KN.search64(X, P, 4)[0], 0.25)
    assert np.allclose(w.sum(1), 1) and (np.diff(w, axis=1) <= 1e-15).all()
    Xr = np.full((3, 7, 8), np.nan, np.float32)
    Xr[0], Xr[2, :4] = X[:7], X[7:11]
    yr, ir, dr = KN.retrieve_ragged64(Xr, [7, 0, 4], P, 4, 0.25)
    assert np.array_equal(yr[0], y[:7]) and np.array_equal(yr[2, :4], y[7:11]) and (yr[1] == 0).all() and (ir[1] == -1).all() and (dr[2, 4:] == 0).all()


def test_units_index_file_and_python_layer_errors(tmp_path):
    from cluster.index import UnitsIndex
    pool = np.random.default_rng(1).standard_normal((20, 16)).astype(np.float32)
    ix = UnitsIndex(pool, source_rows=77, reduced=True)
    ix.save(tmp_path / "units_index.pt")
    ck = torch.load(tmp_path / "units_index.pt", map_location="cpu", weights_only=False)
    assert sorted(ck) == ["n_features_in_", "pool", "reduced", "source_rows"]
    assert isinstance(ck["pool"], np.ndarray) and ck["pool"].dtype == np.float32 and np.array_equal(ck["pool"], pool)
    assert ck["n_features_in_"] == 16 and ck["source_rows"] == 77 and ck["reduced"] is True
    ix2 = UnitsIndex.load(tmp_path / "units_index.pt")
    assert np.array_equal(ix2.pool, pool) and (ix2.n_features_in_, ix2.source_rows, ix2.reduced, len(ix2)) == (16, 77, True, 20)
    assert np.array_equal(UnitsIndex(torch.from_numpy(pool)).state()["pool"], pool) and UnitsIndex(pool).source_rows == 20
    x = torch.zeros(5, 16)
    for call in (lambda: ix.search(x, k=4), lambda: ix.retrieve(x, k=4), lambda: ix.retrieve(x.reshape(1, 5, 16), k=4, lengths=[3])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ix.retrieve(x.numpy())
    for k in (0, 9, 21, 2.5, True):      # (9 > 8; a pool of 20 rows has no 21 neighbours)
        with pytest.raises(ValueError, match="k must be"):
            ix.retrieve(x, k=k)
    with pytest.raises(ValueError, match="k must be"):
        UnitsIndex(pool[:3]).search(x, k=4)
    for ratio in (-0.1, 1.5, float("nan"), "0.5", None):
        with pytest.raises(ValueError, match="ratio"):
            ix.retrieve(x, k=4, ratio=ratio)
    for bad in (torch.zeros(5, 24), torch.zeros(5), torch.zeros(2, 2, 5, 16), torch.zeros(0, 16)):
        with pytest.raises(ValueError, match="against a pool of width 16"):
            ix.retrieve(bad, k=4)
    with pytest.raises(ValueError, match="lengths= needs"):
        ix.retrieve(x, k=4, lengths=[5])
    for lengths in ([6], [-1], [1, 2]):
        with pytest.raises(ValueError, match="lengths must be"):
            ix.retrieve(x.reshape(1, 5, 16), k=4, lengths=lengths)
    with pytest.raises(ValueError, match="at most 64"):
        ix.retrieve(torch.zeros(65, 2, 16), k=4, lengths=[1] * 65)
    for shape in ((20, 12), (20, 4104), (0, 16), (20,)):
        with pytest.raises(ValueError, match="UnitsIndex"):
            UnitsIndex(np.zeros(shape, np.float32))


def test_abi_entries_declared():
    from lds import native
    hdr = open(os.path.join(ROOT, "include", "lds.h")).read()
    for fn in ENTRIES:
        assert fn in native.EXPORTS and fn + "(" in hdr and hasattr(native.lib(), fn)
    assert "lds_test_knn_search" in native.TEST_EXPORTS and "lds_test_knn_search(" in open(os.path.join(ROOT, "include", "lds_test.h")).read()
    assert native.SIGNATURES["lds_knn_retrieve"] == "i:pqppqiifppppzp" and native.SIGNATURES["lds_knn_retrieve_ragged"] == "i:piipppqiifppppzp"
    assert native.SIGNATURES["lds_knn_search"] == "i:pqppqiipppzp" and native.SIGNATURES["lds_test_knn_search"] == "i:pqppqiiiipppzp"
    assert "tools/infer_tools.py:83-117" in hdr.split("units retrieval")[1].split("polyphase")[0]      # the entries cite what they stand in for


def test_limits_answer_before_any_device_call():
    """every limit of the C entries, with null pointers and no workspace: the answer comes before anything touches a device"""
    from lds import native
    L = native.lib()
    err = lambda: L.lds_last_error()      # noqa: E731
    nb = ct.c_size_t(12345)
    wsb = lambda N, M, D, k: L.lds_knn_workspace_bytes(N, M, D, k, ct.byref(nb))      # noqa: E731
    for args, word in (((10, 100, 12, 4), b"D 12"), ((10, 100, 4, 4), b"D 4"), ((10, 100, 4104, 4), b"D 4104"), ((10, 100, 16, 0), b"k 0"),
                       ((10, 100, 16, 9), b"k 9"), ((10, 3, 16, 4), b"k 4"), ((10, 0, 16, 1), b"M 0"), ((10, 16777217, 16, 4), b"M 16777217"),
                       ((0, 100, 16, 4), b"N 0"), ((2147483001, 100, 16, 4), b"N 2147483001")):
        assert wsb(*args) == -1 and word in err() and nb.value == 12345, args
    assert L.lds_knn_workspace_bytes(10, 100, 16, 4, None) == -1
    # N = 129 rows against M = 1000 (8 pool blocks, one split each), lists of 4 for k = 3: two arrays [8][129][4] of 4 bytes, each rounded to 256
    assert wsb(129, 1000, 64, 3) == 0 and nb.value == 2 * ((8 * 129 * 4 * 4 + 255) // 256 * 256)
    assert wsb(2147483000, 16777216, 4096, 8) == 0 and nb.value >= 2147483000 * 8 * 8
    assert L.lds_knn_prepare(None, 100, 12, None, None) == -1 and b"D 12" in err()
    assert L.lds_knn_prepare(None, 100, 16, None, None) == -1 and b"null" in err()
    assert L.lds_knn_search(None, 10, None, None, 100, 16, 9, None, None, None, 0, None) == -1 and b"k 9" in err()
    assert L.lds_knn_search(None, 10, None, None, 100, 16, 4, None, None, None, 0, None) == -1 and b"null" in err()
    for ratio in (-0.01, 1.01, float("nan")):
        assert L.lds_knn_retrieve(None, 10, None, None, 100, 16, 4, ratio, None, None, None, None, 0, None) == -1 and b"ratio" in err()
    assert L.lds_knn_retrieve(None, 10, None, None, 100, 20, 4, 0.5, None, None, None, None, 0, None) == -1 and b"D 20" in err()
    assert L.lds_knn_retrieve(None, 10, None, None, 100, 16, 4, 0.5, None, None, None, None, 0, None) == -1 and b"null" in err()
    ln = (ct.c_int32 * 2)(3, 6)
    rag = lambda B, T, lengths, k=4: L.lds_knn_retrieve_ragged(None, B, T, lengths, None, None, 100, 16, k, 0.5, None, None, None, None, 0, None)      # noqa: E731
    assert rag(65, 5, ln) == -1 and b"B 65" in err()
    assert rag(2, 0, ln) == -1 and b"T 0" in err()
    assert rag(2, 5, None) == -1 and b"null lengths" in err()
    assert rag(2, 5, ct.cast(ln, ct.c_void_p)) == -1 and b"lengths[1] = 6" in err()
    assert rag(2, 6, ct.cast(ln, ct.c_void_p), k=9) == -1 and b"k 9" in err()
    assert rag(2, 6, ct.cast(ln, ct.c_void_p)) == -1 and b"null pointer" in err()
    # a short workspace and a misaligned tensor are refused before the first launch: the addresses are never followed
    fake = 1 << 20
    assert L.lds_knn_search(fake, 10, fake, fake, 100, 16, 4, fake, None, fake, 255, None) == -2 and b"512" in err()
    assert L.lds_knn_retrieve(fake, 10, fake, fake, 100, 16, 4, 0.5, fake, None, None, fake, 0, None) == -2
    assert L.lds_knn_search(fake + 4, 10, fake, fake, 100, 16, 4, fake, None, fake, 1 << 20, None) == -1 and b"aligned" in err()
    for slab, splits, word in ((100, 1, b"slab_rows"), (0, 1, b"slab_rows"), (128, 0, b"splits"), (128, 65, b"splits")):
        assert L.lds_test_knn_search(None, 10, None, None, 100, 16, 4, slab, splits, None, None, None, 0, None) == -1 and word in err()
    assert L.lds_test_knn_search(fake, 10, fake, fake, 333, 16, 8, 128, 3, fake, None, fake, 100, None) == -2


def _tool():
    spec = importlib.util.spec_from_file_location("train_units_index", os.path.join(ROOT, "tools", "train_units_index.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_units_index_reduction_rule(tmp_path, monkeypatch, capsys):
    tool = _tool()
    calls = []

    def stub(features, n_clusters, max_iter=500, tol=1e-2, **kw):      # cluster.train_cluster's checkpoint dict, without a device
        calls.append((features.shape, n_clusters, max_iter))
        return {"n_features_in_": features.shape[1], "_n_threads": 4, "cluster_centers_": features[:n_clusters].astype(np.float64) + 1}
    monkeypatch.setattr(tool.cluster, "train_cluster", stub)
    feats = np.random.default_rng(2).standard_normal((100, 16)).astype(np.float32)
    pool, reduced = tool.build_pool(feats, 100, 10)      # up to max_rows: the frames themselves, nothing is fitted
    assert not reduced and np.array_equal(pool, feats) and not calls
    pool, reduced = tool.build_pool(feats, 99, 10, max_iter=7)
    assert reduced and pool.dtype == np.float32 and np.array_equal(pool, feats[:10] + 1) and calls == [((100, 16), 10, 7)]
    with pytest.raises(ValueError, match="reduce_to"):
        tool.build_pool(feats, 50, 51)
    udir = tmp_path / "units" / "spk"
    udir.mkdir(parents=True)
    np.save(udir / "a.npy", feats[:60])
    np.save(udir / "b.npy", feats[60:])
    from cluster.index import UnitsIndex
    tool.main([str(tmp_path / "units"), "-o", str(tmp_path / "whole.pt")])
    ix = UnitsIndex.load(tmp_path / "whole.pt")
    assert (len(ix), ix.source_rows, ix.reduced) == (100, 100, False) and sorted(map(tuple, ix.pool)) == sorted(map(tuple, feats))
    tool.main([str(tmp_path / "units"), "-o", str(tmp_path / "reduced.pt"), "--max_rows", "80", "--reduce_to", "12"])
    ix = UnitsIndex.load(tmp_path / "reduced.pt")
    assert (len(ix), ix.source_rows, ix.reduced, ix.n_features_in_) == (12, 100, True, 16) and calls[-1][:2] == ((100, 16), 12)
    tool.main([str(tmp_path / "units"), "-o", str(tmp_path / "syn.pt"), "--synthetic", "40"])
    ix = UnitsIndex.load(tmp_path / "syn.pt")
    assert (len(ix), ix.source_rows, ix.reduced) == (40, 100, False)
    with pytest.raises(SystemExit):
        tool.main([str(tmp_path / "nowhere"), "-o", str(tmp_path / "x.pt")])


@pytest.mark.parametrize("case", KN.GAUSSIAN, ids=lambda c: "x".join(map(str, c)))
def test_fp32_scores_attain_the_gpu_tests_cap(case):
    """On the inputs of tests/test_gpu_knn.py's Gaussian cases a plain numpy fp32 evaluation of the scores gives index lists that differ from the
    float64 oracle's in at most 0.5 % of the rows: the GPU test's cap of 2 % is within reach of fp32 arithmetic (measured here: 0 rows of 257
    and 0 rows of 64 -- a near-tie inside fp32's resolution is rare among 8 of thousands of Gaussian rows)."""
    N, M, D, k = case
    X, P = KN.gaussian_case(N, M, D)
    idx64, _ = KN.search64(X, P, k)
    idx32 = KN.topk_stable(KN.scores(X, P, np.float32), k)
    differing = int((idx32 != idx64).any(1).sum())
    print(f"{case}: rows whose fp32 list differs from float64's: {differing} of {N}")
    assert differing <= 0.005 * N
    # and the distances those fp32 lists stand for sit inside the search bound of the same rank
    assert (np.abs(KN.dist64(X, P, idx32) - KN.dist64(X, P, idx64)) <= KN.search_bound(X, P)[:, None]).all()
