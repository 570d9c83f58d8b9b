"""Units retrieval through the IVF coarse index without a GPU: the restatement (tests/ivf_numpy.py) against knn_numpy's exact search, the
UnitsIndex file with and without the "ivf" key, the Python-layer refusals and the C entries' limits (they answer before any device work),
the ABI, the index tool's --nlist path with a stubbed fit, and what fp32 arithmetic attains on the inputs tests/test_gpu_ivf.py uses."""
import ctypes as ct
import importlib.util
import os

import numpy as np
import pytest

import ivf_numpy as IV
import knn_numpy as KN
from conftest import ROOT

torch = pytest.importorskip("torch")

ENTRIES = ("lds_ivf_workspace_bytes", "lds_ivf_search", "lds_ivf_retrieve", "lds_ivf_retrieve_ragged")


def numpy_assign(pool, centres, device):
    """stands in for cluster.index._assign_lists (lds_kmeans_assign on the device) where there is no device"""
    return np.argmax(KN.scores(np.asarray(pool), np.asarray(centres)), axis=1)


@pytest.mark.parametrize("case", IV.LATTICE, ids=lambda c: "x".join(map(str, c)))
def test_all_lists_probed_is_the_exact_search(case):
    N, M, D, k, L, nprobe = case
    X, P = KN.lattice_case(N, M, D)
    ivf = IV.build(P, IV.lattice_centres(L, D))
    centres, offsets, order = ivf
    assert offsets[0] == 0 and offsets[-1] == M and (np.diff(offsets) >= 1).all() and np.array_equal(np.sort(order), np.arange(M))
    assert all((np.diff(order[a:b]) > 0).all() for a, b in zip(offsets[:-1], offsets[1:]))      # ascending original index inside a list
    idx, sc = IV.search(X, P, k, ivf, len(centres))
    want, score = KN.search64(X, P, k)
    assert np.array_equal(idx, want) and np.array_equal(sc, score)
    part, psc = IV.search(X, P, k, ivf, min(nprobe, len(centres)))
    assert (psc <= sc).all() and ((part >= 0) == np.isfinite(psc)).all()


def test_empty_lists_are_dropped():
    X, P = KN.lattice_case(20, 50, 8)
    C = IV.lattice_centres(4, 8)
    far = np.full((2, 8), 100.0, np.float32)      # score p.c - 400 |c|^2-wise: never the best centre of a row in -3 .. 3
    centres, offsets, order = IV.build(P, np.concatenate([C[:2], far[:1], C[2:], far[1:]]))
    ref = IV.build(P, C)
    assert np.array_equal(centres, ref[0]) and np.array_equal(offsets, ref[1]) and np.array_equal(order, ref[2]) and len(centres) <= 4


def test_fewer_candidates_than_k_get_the_fill():
    case = IV.LATTICE[1]      # 8 pool rows in 3 lists
    N, M, D, k, L, nprobe = case
    X, P = KN.lattice_case(N, M, D)
    ivf = IV.build(P, IV.lattice_centres(L, D))
    idx, sc = IV.search(X, P, 8, ivf, 1)
    lens = np.diff(ivf[1])[IV.probe(X, ivf[0], 1)[:, 0]]
    assert lens.max() < 8
    for r, s, n in zip(idx, sc, lens):
        assert (r[:n] >= 0).all() and (r[n:] == -1).all() and np.isneginf(s[n:]).all() and np.isfinite(s[:n]).all() and (np.diff(s[:n]) <= 0).all()
    y, d, w = IV.blend64(X, P, idx, 0.5)
    assert np.isfinite(y).all() and np.allclose(w.sum(1), 1) and (w[idx < 0] == 0).all() and (d[idx < 0] == 0).all()
    full = KN.search64(X, P, 8)[0]
    assert np.allclose(IV.blend64(X, P, full, 0.25)[0], KN.blend64(X, P, full, 0.25)[0], rtol=0, atol=1e-12)      # nothing missing: knn_numpy's blend


def test_ties_go_by_original_index_across_lists():
    """the triplicated pool of tests/test_gpu_ivf.py: a tag column sends each copy of a row to its own list; queries without the tag score
    the three copies equally and must get them in original order"""
    X, P = KN.lattice_case(130, 100, 24)
    tag = np.zeros((300, 8), np.float32)
    tag[np.arange(300), np.arange(300) // 100] = 40.0
    P3 = np.concatenate([np.concatenate([P, P, P]), tag], 1)
    C = np.zeros((3, 32), np.float32)
    C[np.arange(3), 24 + np.arange(3)] = 40.0
    X3 = np.concatenate([X, np.zeros((130, 8), np.float32)], 1)
    ivf = IV.build(P3, C)
    assert np.array_equal(np.diff(ivf[1]), [100, 100, 100]) and np.array_equal(ivf[2], np.arange(300))
    idx, sc = IV.search(X3, P3, 8, ivf, 3)
    assert np.array_equal(idx, KN.search64(X3, P3, 8)[0]) and (sc[:, :3] == sc[:, :1]).all() and (np.diff(idx[:, :3], axis=1) > 0).all()
    two, _ = IV.search(X3, P3, 8, ivf, 2)      # two of the three lists: only their copies
    pl = IV.probe(X3, ivf[0], 2)
    assert all(set(r // 100) <= set(p) for r, p in zip(two, pl))


def test_state_round_trip_with_and_without_ivf(tmp_path, monkeypatch):
    import cluster.index as CI
    monkeypatch.setattr(CI, "_assign_lists", numpy_assign)
    pool = np.random.default_rng(1).standard_normal((40, 16)).astype(np.float32)
    plain = CI.UnitsIndex(pool)
    assert sorted(plain.state()) == ["n_features_in_", "pool", "reduced", "source_rows"] and plain.nlist == 0 and plain.ivf is None
    plain.save(tmp_path / "plain.pt")
    assert CI.UnitsIndex.load(tmp_path / "plain.pt").ivf is None
    C = np.concatenate([IV.gaussian_centres(5, 16), np.full((1, 16), 50.0, np.float32)])      # the sixth centre receives no row
    ix = CI.UnitsIndex(pool, source_rows=90).build_ivf(6, centres=C)
    ref = IV.build(pool, C)
    assert ix.nlist == len(ref[0]) <= 5
    st = ix.state()
    assert sorted(st) == ["ivf", "n_features_in_", "pool", "reduced", "source_rows"] and sorted(st["ivf"]) == ["centres", "offsets", "order"]
    assert st["ivf"]["centres"].dtype == np.float32 and st["ivf"]["offsets"].dtype == np.int64 and st["ivf"]["order"].dtype == np.int32
    assert all(np.array_equal(st["ivf"][n], a) for n, a in zip(("centres", "offsets", "order"), ref))
    ix.save(tmp_path / "ivf.pt")
    ck = torch.load(tmp_path / "ivf.pt", map_location="cpu", weights_only=False)
    assert all(isinstance(ck["ivf"][n], np.ndarray) for n in ("centres", "offsets", "order"))
    ix2 = CI.UnitsIndex.load(tmp_path / "ivf.pt")
    assert ix2.nlist == ix.nlist and ix2.source_rows == 90 and all(np.array_equal(ix2.ivf[n], ix.ivf[n]) for n in ix.ivf)
    ck["ivf"]["offsets"] = ck["ivf"]["offsets"][::-1].copy()
    torch.save(ck, tmp_path / "broken.pt")
    with pytest.raises(ValueError, match="IVF tables"):
        CI.UnitsIndex.load(tmp_path / "broken.pt")
    for nlist, centres in ((0, None), (41, None), (65537, None), (2.5, None), (True, None), (3, C), (6, C[:, :8])):
        with pytest.raises(ValueError, match="nlist must be|centres"):
            CI.UnitsIndex(pool).build_ivf(nlist, centres=centres)


def test_refusals_before_any_device_work(monkeypatch):
    import cluster.index as CI
    pool = np.random.default_rng(1).standard_normal((40, 16)).astype(np.float32)
    x = torch.zeros(5, 16)
    plain = CI.UnitsIndex(pool)
    for call in (lambda: plain.search(x, k=4, nprobe=1), lambda: plain.retrieve(x, k=4, nprobe=1), lambda: plain.probe_lists(x, 1)):
        with pytest.raises(ValueError, match="needs an IVF"):
            call()
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # the real assignment runs on the device only
        CI.UnitsIndex(pool).build_ivf(4, centres=IV.gaussian_centres(4, 16), device="cpu")
    monkeypatch.setattr(CI, "_assign_lists", numpy_assign)
    ix = CI.UnitsIndex(pool).build_ivf(4, centres=IV.gaussian_centres(4, 16))
    assert ix.nlist == 4
    for nprobe in (0, 9, 5, 2.0, True, "1"):      # (9 > 8; four lists have no fifth)
        for call in (lambda: ix.search(x, k=4, nprobe=nprobe), lambda: ix.retrieve(x, k=4, nprobe=nprobe), lambda: ix.probe_lists(x, nprobe)):
            with pytest.raises(ValueError, match="nprobe must be"):
                call()
    for call in (lambda: ix.search(x, k=4, nprobe=2), lambda: ix.retrieve(x, k=4, nprobe=2), lambda: ix.probe_lists(x, 2),
                 lambda: ix.retrieve(x.reshape(1, 5, 16), k=4, lengths=[3], nprobe=2)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ix.probe_lists(x.numpy(), 2)
    with pytest.raises(ValueError, match="k must be"):
        ix.search(x, k=9, nprobe=2)
    with pytest.raises(ValueError, match="against a pool of width 16"):
        ix.probe_lists(torch.zeros(5, 24), 2)


def test_abi_entries_declared():
    from lds import native
    hdr = open(os.path.join(ROOT, "include", "lds.h")).read()
    for fn in ENTRIES:
        assert fn in native.EXPORTS and fn + "(" in hdr and hasattr(native.lib(), fn)
    assert "lds_test_ivf_search" in native.TEST_EXPORTS and "lds_test_ivf_search(" in open(os.path.join(ROOT, "include", "lds_test.h")).read()
    index = "ppippppqi"      # C, hc, nlist, offsets, order, PL, hl, copy_rows, nprobe
    assert native.SIGNATURES["lds_ivf_workspace_bytes"] == "i:qqiiiip"
    for ivf, knn, at in (("lds_ivf_search", "lds_knn_search", 7), ("lds_ivf_retrieve", "lds_knn_retrieve", 7), ("lds_ivf_retrieve_ragged", "lds_knn_retrieve_ragged", 9)):
        sig = native.SIGNATURES[knn]      # the counterpart's arguments with the index after k
        assert native.SIGNATURES[ivf] == sig[:2 + at] + index + sig[2 + at:], ivf
    sig = native.SIGNATURES["lds_knn_search"]
    assert native.SIGNATURES["lds_test_ivf_search"] == sig[:9] + index + "i" + sig[9:]
    assert "IndexIVFFlat" in hdr.split("IVF coarse index")[1].split("polyphase")[0]      # the entries cite what they stand in for


def test_limits_answer_before_any_device_call():
    """every limit of the C entries, with null or never-followed pointers and no workspace: the answer comes before anything touches a device"""
    from lds import native
    L = native.lib()
    err = lambda: L.lds_last_error()      # noqa: E731
    nb = ct.c_size_t(12345)
    wsb = lambda *a: L.lds_ivf_workspace_bytes(*a, ct.byref(nb))      # noqa: E731
    for args, word in (((10, 100, 12, 4, 8, 2), b"D 12"), ((10, 100, 16, 9, 8, 2), b"k 9"), ((10, 0, 16, 1, 1, 1), b"M 0"), ((0, 100, 16, 4, 8, 2), b"N 0"),
                       ((10, 100, 16, 4, 0, 1), b"nlist 0"), ((10, 100, 16, 4, 65537, 1), b"nlist 65537"), ((10, 100, 16, 4, 101, 1), b"nlist 101"),
                       ((10, 100, 16, 4, 8, 0), b"nprobe 0"), ((10, 100, 16, 4, 16, 9), b"nprobe 9"), ((10, 100, 16, 4, 3, 4), b"nprobe 4"),
                       ((2147418112 // (4096 * 4) + 1, 100, 4096, 4, 8, 2), b"one descriptor")):
        assert wsb(*args) == -1 and word in err() and nb.value == 12345, args
    assert L.lds_ivf_workspace_bytes(10, 100, 16, 4, 8, 2, None) == -1
    assert wsb(2147418112 // (4096 * 4), 100, 4096, 4, 8, 2) == 0
    # N = 129, M = 1000, k = 3 (lists of 4), 16 lists, 8 probed: the per-(query, probe slot) lists alone are two arrays [8][129][4] of 4 bytes
    assert wsb(129, 1000, 64, 3, 16, 8) == 0 and nb.value >= 2 * 8 * 129 * 4 * 4 + 129 * 8 * (4 + 8)
    need = nb.value
    fake = 1 << 20
    index = (fake, fake, 16, fake, fake, fake, fake, 1024, 8)      # C, hc, nlist, offsets, order, PL, hl, copy_rows, nprobe

    def search(N=129, M=1000, D=64, k=3, ix=index, x=fake, ws=fake, ws_bytes=need, test=False):
        if test is not False:
            return L.lds_test_ivf_search(x, N, None, None, M, D, k, *ix, test, fake, None, ws, ws_bytes, None)
        return L.lds_ivf_search(x, N, None, None, M, D, k, *ix, fake, None, ws, ws_bytes, None)

    def retrieve(N=129, M=1000, D=64, k=3, ix=index, ratio=0.5, x=fake, y=fake, ws_bytes=need, lengths=None, B=3, T=43):
        if lengths is not None:
            return L.lds_ivf_retrieve_ragged(x, B, T, lengths, fake, None, M, D, k, *ix, ratio, y, None, None, fake, ws_bytes, None)
        return L.lds_ivf_retrieve(x, N, fake, None, M, D, k, *ix, ratio, y, None, None, fake, ws_bytes, None)

    def with_(at, v):
        return index[:at] + (v,) + index[at + 1:]
    for fn in (search, retrieve):
        assert fn(D=20) == -1 and b"D 20" in err()
        assert fn(k=9) == -1 and b"k 9" in err()
        assert fn(ix=with_(8, 0)) == -1 and b"nprobe 0" in err()
        assert fn(ix=with_(8, 9)) == -1 and b"nprobe 9" in err()
        assert fn(ix=with_(2, 7)) == -1 and b"nprobe 8" in err()
        assert fn(ix=with_(2, 65537)) == -1 and b"nlist 65537" in err()
        assert fn(x=None) == -1 and b"null" in err()
        for at in (0, 1, 3, 4, 5, 6):
            assert fn(ix=with_(at, None)) == -1 and b"null pointer in the index" in err()
        assert fn(ix=with_(0, fake + 4)) == -1 and b"aligned" in err()
        assert fn(ix=with_(5, fake + 8)) == -1 and b"aligned" in err()
        assert fn(x=fake + 4) == -1 and b"aligned" in err()
        for rows in (896, 1000, 1024 + 16 * 128):      # below M, no multiple of 128, beyond M + 127 nlist
            assert fn(ix=with_(7, rows)) == -1 and b"copy_rows" in err()
        assert fn(ws_bytes=need - 1) == -2 and str(need).encode() in err()
    for ratio in (-0.01, 1.01, float("nan")):
        assert retrieve(ratio=ratio) == -1 and b"ratio" in err()
    assert retrieve(y=None) == -1 and b"null" in err()
    ln = (ct.c_int32 * 3)(3, 44, 0)
    assert retrieve(lengths=ct.cast(ln, ct.c_void_p)) == -1 and b"lengths[1] = 44" in err()
    assert retrieve(lengths=ct.cast(ln, ct.c_void_p), B=65) == -1 and b"B 65" in err()
    assert L.lds_ivf_retrieve_ragged(fake, 3, 43, None, fake, None, 1000, 64, 3, *index, 0.5, fake, None, None, fake, need, None) == -1 and b"null lengths" in err()
    for slab in (0, 100, 129):
        assert search(test=slab) == -1 and b"slab_rows" in err()
    assert search(test=128, ws_bytes=need - 1) == -2


def _tool():
    spec = importlib.util.spec_from_file_location("train_units_index", os.path.join(ROOT, "tools", "train_units_index.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_units_index_nlist_path(tmp_path, monkeypatch):
    import cluster.index as CI
    tool = _tool()
    calls = []

    def stub(features, n_clusters, max_iter=500, tol=1e-2, **kw):      # cluster.train_cluster's checkpoint dict, without a device
        calls.append((features.shape, n_clusters, max_iter))
        return {"n_features_in_": features.shape[1], "_n_threads": 4, "cluster_centers_": np.asarray(features[:n_clusters], np.float64) + 0.25}
    monkeypatch.setattr(tool.cluster, "train_cluster", stub)
    monkeypatch.setattr(CI, "_assign_lists", numpy_assign)
    feats = np.random.default_rng(2).standard_normal((100, 16)).astype(np.float32)
    udir = tmp_path / "units" / "spk"
    udir.mkdir(parents=True)
    np.save(udir / "a.npy", feats)
    tool.main([str(tmp_path / "units"), "-o", str(tmp_path / "plain.pt")])      # the default: no IVF, the four keys, nothing fitted
    assert sorted(torch.load(tmp_path / "plain.pt", weights_only=False)) == ["n_features_in_", "pool", "reduced", "source_rows"] and not calls
    tool.main([str(tmp_path / "units"), "-o", str(tmp_path / "ivf.pt"), "--nlist", "7", "--nlist_iter", "3"])
    ix = CI.UnitsIndex.load(tmp_path / "ivf.pt")
    assert calls == [((100, 16), 7, 3)] and (len(ix), ix.source_rows, ix.reduced, ix.nlist) == (100, 100, False, 7)
    ref = IV.build(ix.pool, ix.pool[:7] + np.float32(0.25))
    assert all(np.array_equal(ix.ivf[n], a) for n, a in zip(("centres", "offsets", "order"), ref))
    for bad in ("101", "-1", "65537"):
        with pytest.raises(SystemExit):
            tool.main([str(tmp_path / "units"), "-o", str(tmp_path / "x.pt"), "--nlist", bad])


@pytest.mark.parametrize("nprobe", IV.GAUSSIAN_NPROBE)
def test_fp32_attains_the_gpu_tests_cap(nprobe):
    """On the inputs of tests/test_gpu_ivf.py's Gaussian cases (KN.GAUSSIAN[0], 16 seeded Gaussian centres) a plain numpy fp32 evaluation of
    the build, the probe and the search differs from float64's in at most 0.5 % of the rows -- rows whose probed lists differ plus rows whose
    neighbour list differs: the GPU test's cap of 2 % is within reach of fp32 arithmetic (measured here: 0 rows of 257 at nprobe 1 and 0 at
    nprobe 4, no pool row in another list)."""
    N, M, D, k = KN.GAUSSIAN[0]
    X, P = KN.gaussian_case(N, M, D)
    C = IV.gaussian_centres(IV.GAUSSIAN_CENTRES, D)
    ivf64, ivf32 = IV.build(P, C), IV.build(P, C, np.float32)
    moved = int((ivf64[2] != ivf32[2]).sum()) if len(ivf64[0]) == len(ivf32[0]) else M
    probes = (IV.probe(X, ivf64[0], nprobe) != IV.probe(X, ivf64[0], nprobe, np.float32)).any(1)
    idx64, _ = IV.search(X, P, k, ivf64, nprobe)
    idx32, _ = IV.search(X, P, k, ivf64, nprobe, np.float32)
    differing = int(((idx32 != idx64).any(1) | probes).sum())
    print(f"nprobe {nprobe}: pool rows in another list {moved} of {M}; rows with other probed lists {int(probes.sum())}, with other lists or neighbours "
          f"{differing} of {N}")
    assert len(ivf64[0]) == IV.GAUSSIAN_CENTRES and (idx64 >= 0).all()
    assert moved == 0 and differing <= 0.005 * N
    assert (np.abs(KN.dist64(X, P, idx32) - KN.dist64(X, P, idx64))[~probes] <= KN.search_bound(X, P)[~probes, None]).all()
