"""Units retrieval through the IVF coarse index on a real MI355X (csrc/knn.hip's ivf_* kernels through lds.native and
cluster.index.UnitsIndex) against the restatement of tests/ivf_numpy.py: exact lists and scores on lattice inputs (short lists, ragged last
blocks, lists in different slabs, ties across lists), nprobe = nlist against the exact path bit for bit, the a-priori distance bound on
Gaussian inputs, buckets of more than 128 queries, bit-for-bit invariances, the limits, corrupt tables, and the pipeline."""
import ctypes as ct
import functools

import numpy as np
import pytest

import ivf_numpy as IV
import knn_numpy as KN

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NAN_WORD, X7F_WORD = 0x7FC00000, 0x7F7F7F7F


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()      # (a copy: the shared inputs are read-only)


def bits(t):
    return t.contiguous().view(torch.int32)


def built(P, centres, exact=True):
    """(the UnitsIndex with lists from `centres`, the tables the restatement searches).  exact (lattice inputs: every assign score is exact):
    the index's tables must be the restatement's own build; otherwise the search is restated on the lists the index holds -- a pool row
    between two centres within fp32's resolution may sit in either -- and the rows that IV.build places elsewhere are printed."""
    from cluster.index import UnitsIndex
    ix = UnitsIndex(np.array(P)).build_ivf(len(centres), centres=centres)
    ivf = IV.build(P, centres)
    if exact:
        assert ix.nlist == len(ivf[0]) and all(np.array_equal(ix.ivf[n], a) for n, a in zip(("centres", "offsets", "order"), ivf))
        return ix, ivf
    print(f"pool rows whose list differs from the float64 build's: {int((ix.ivf['order'] != ivf[2]).sum()) if len(ivf[2]) == len(ix.ivf['order']) else '?'}")
    return ix, (ix.ivf["centres"], ix.ivf["offsets"], ix.ivf["order"])


@functools.lru_cache(maxsize=None)
def lattice(case):
    N, M, D, k, L, nprobe = case
    X, P = KN.lattice_case(N, M, D)
    ix, ivf = built(P, IV.lattice_centres(L, D))
    return X, P, ix, ivf


@functools.lru_cache(maxsize=None)
def gaussian():
    """(X, P, index, tables) of KN.GAUSSIAN[0] with 16 seeded Gaussian centres: computed once, shared, never written to"""
    N, M, D, k = KN.GAUSSIAN[0]
    X, P = KN.gaussian_case(N, M, D)
    ix, ivf = built(P, IV.gaussian_centres(IV.GAUSSIAN_CENTRES, D), exact=False)
    for a in (X, P):
        a.setflags(write=False)
    return X, P, ix, ivf


def same_lists(idx, sc, want, score):
    return np.array_equal(idx.cpu().numpy(), want) and np.array_equal(sc.cpu().numpy().astype(np.float64), score)


# ---- lattice cases: every score exact in fp32, so lists and scores are the restatement's, rank by rank and bit by bit ----
@pytest.mark.parametrize("case", IV.LATTICE, ids=lambda c: "x".join(map(str, c)))
def test_lattice_exact(case):
    N, M, D, k, L, nprobe = case
    X, P, ix, ivf = lattice(case)
    nprobe = min(nprobe, ix.nlist)
    want, score = IV.search(X, P, k, ivf, nprobe)
    Xd = dev(X)
    assert np.array_equal(ix.probe_lists(Xd, nprobe).cpu().numpy(), IV.probe(X, ivf[0], nprobe))
    idx, sc = ix.search(Xd, k=k, nprobe=nprobe)
    assert idx.dtype == torch.int64 and idx.shape == (N, k) and same_lists(idx, sc, want, score)
    y, ri, rd = ix.retrieve(Xd, k=k, ratio=0.5, return_neighbours=True, nprobe=nprobe)
    assert np.array_equal(ri.cpu().numpy(), want)
    y64, d64, _ = IV.blend64(X, P, want, 0.5)      # the blend over the entries found: -1 has weight 0
    assert torch.isfinite(y).all() and (np.abs(y.cpu().numpy() - y64) <= KN.blend_bound(X, P)).all()
    d64 = np.where(d64 == KN.FLOOR, float(np.float32(KN.FLOOR)), d64)      # (a query that is a pool row: the fp32 floor)
    assert np.array_equal(rd.cpu().numpy()[want >= 0].astype(np.float64), d64[want >= 0])      # (sums of integer squares: exact)


def test_lattice_short_lists_fill():
    """129 x 8 x 8, k 8, one probed list: no list holds 8 rows, so every query has -1 / -inf behind its list's rows"""
    case = IV.LATTICE[1]
    X, P, ix, ivf = lattice(case)
    idx, sc = ix.search(dev(X), k=8, nprobe=1)
    idx, sc = idx.cpu().numpy(), sc.cpu().numpy()
    lens = np.diff(ivf[1])[IV.probe(X, ivf[0], 1)[:, 0]]
    assert lens.max() < 8 and all((r[:n] >= 0).all() and (r[n:] == -1).all() for r, n in zip(idx, lens)) and np.array_equal(idx == -1, np.isneginf(sc))


def test_lattice_triplicated_pool():
    """tests/test_gpu_knn.py's triplicated pool: the three copies of a row tie exactly and fall into different lists (each copy carries a tag
    column that sends it to its own centre); they come lowest original index first across the lists"""
    X, P = KN.lattice_case(130, 100, 24)
    tag = np.zeros((300, 8), np.float32)
    tag[np.arange(300), np.arange(300) // 100] = 40.0
    P3 = np.concatenate([np.concatenate([P, P, P]), tag], 1)
    C = np.zeros((3, 32), np.float32)
    C[np.arange(3), 24 + np.arange(3)] = 40.0
    X3 = np.concatenate([X, np.zeros((130, 8), np.float32)], 1)      # the queries see no tag: equal scores for the three copies
    ix, ivf = built(P3, C)
    assert np.array_equal(np.diff(ivf[1]), [100, 100, 100])
    want, score = IV.search(X3, P3, 8, ivf, 3)
    assert np.array_equal(want, KN.search64(X3, P3, 8)[0]) and (want[:, 0] < 100).all() and (np.diff(want[:, :3], axis=1) > 0).all()
    idx, sc = ix.search(dev(X3), k=8, nprobe=3)
    assert same_lists(idx, sc, want, score)


def test_lattice_lists_in_different_slabs():
    """M 333 through lds_test_ivf_search with slab_rows 128: every 128-row block of the list-ordered copy behind a descriptor of its own"""
    from lds import native
    case = IV.LATTICE[5]
    N, M, D, k, L, nprobe = case
    X, P, ix, ivf = lattice(case)
    Xd = dev(X)
    pool, h = ix._device(Xd.device)
    on = ix._device_ivf(Xd.device)
    assert on[4].shape[0] > 256
    ws = torch.empty(native.ivf_workspace_bytes(N, M, D, k, ix.nlist, nprobe), dtype=torch.uint8, device="cuda")
    native.debug_fill(ws, NAN_WORD)
    idx, sc = native.ivf_search(Xd, pool, h, k, on, nprobe, ws=ws, slab_rows=128)
    assert same_lists(idx, sc, *IV.search(X, P, k, ivf, nprobe))


# ---- nprobe = nlist: the exact path's lists, scores and blend, bit for bit ----
@pytest.mark.parametrize("case", [c for c in IV.LATTICE if c[4] <= 8], ids=lambda c: "x".join(map(str, c)))
def test_all_lists_probed_equals_the_exact_path(case):
    N, M, D, k, L, nprobe = case
    X, P, ix, ivf = lattice(case)
    Xd = dev(X)
    a, b = ix.search(Xd, k=k, nprobe=ix.nlist), ix.search(Xd, k=k)
    assert torch.equal(a[0], b[0]) and torch.equal(bits(a[1]), bits(b[1]))
    ya, yb = ix.retrieve(Xd, k=k, ratio=0.5, nprobe=ix.nlist), ix.retrieve(Xd, k=k, ratio=0.5)
    assert torch.equal(bits(ya), bits(yb))


# ---- Gaussian cases: the a-priori bound ----
@pytest.mark.parametrize("nprobe", IV.GAUSSIAN_NPROBE)
def test_gaussian_within_search_bound(nprobe, record_margin):
    """rows whose probed lists differ from float64's count towards the cap and are left out; on the others every returned neighbour's true
    (float64) distance equals the restatement's of the same rank within E_n (knn_numpy.search_bound); indices distinct and inside [0, M); rows
    whose list differs plus rows left out: at most 2 % (tests/test_cpu_ivf.py: fp32 itself stays under 0.5 % on these inputs)"""
    N, M, D, k = KN.GAUSSIAN[0]
    X, P, ix, ivf = gaussian()
    Xd = dev(X)
    same = (ix.probe_lists(Xd, nprobe).cpu().numpy() == IV.probe(X, ivf[0], nprobe)).all(1)
    idx, score = ix.search(Xd, k=k, nprobe=nprobe)
    idx = idx.cpu().numpy()
    want, _ = IV.search(X, P, k, ivf, nprobe)
    assert (want >= 0).all()      # (lists of hundreds of rows: every query finds k)
    assert idx.min() >= 0 and idx.max() < M and all(len(set(r)) == k for r in idx)
    E = KN.search_bound(X, P)
    err = np.abs(KN.dist64(X, P, idx) - KN.dist64(X, P, want)) / E[:, None]
    worst = float(err[same].max())
    differing = int((idx != want).any(1)[same].sum()) + int((~same).sum())
    print(f"nprobe {nprobe}: worst distance error / E_n {worst:.3g}; rows left out (other probed lists) {int((~same).sum())}, "
          f"rows left out or with another list than float64's: {differing} of {N}")
    record_margin(worst, 1.0)
    assert differing <= 0.02 * N
    x2 = (X.astype(np.float64) ** 2).sum(1)[:, None]
    assert (np.abs(x2 - 2 * score.cpu().numpy() - KN.dist64(X, P, idx)) <= E[:, None]).all()      # the scores are the winners' own


# ---- buckets ----
def test_bucket_of_300_identical_queries():
    """300 copies of one query: its probed lists' buckets hold 300 entries (three workgroups each), every other list's none; all rows equal
    the single-row call"""
    X, P, ix, ivf = gaussian()
    Xd = dev(np.repeat(X[5:6], 300, 0))
    assert ix.nlist > 2 and (ix.probe_lists(Xd, 2) == ix.probe_lists(Xd[:1], 2)).all()
    y, idx, dist = ix.retrieve(Xd, k=8, ratio=0.5, return_neighbours=True, nprobe=2)
    y1, i1, d1 = ix.retrieve(Xd[:1].contiguous(), k=8, ratio=0.5, return_neighbours=True, nprobe=2)
    assert (idx == i1).all() and (bits(dist) == bits(d1)).all() and (bits(y) == bits(y1)).all()
    assert np.array_equal(i1.cpu().numpy(), IV.search(X[5:6], P, 8, ivf, 2)[0])


def test_permuted_queries_and_row_as_if_alone():
    X, P, ix, ivf = gaussian()
    Xd = dev(X)
    y, idx, dist = ix.retrieve(Xd, k=8, ratio=0.5, return_neighbours=True, nprobe=4)
    s_idx, s_sc = ix.search(Xd, k=8, nprobe=4)
    assert torch.equal(s_idx, idx)
    perm = torch.from_numpy(np.random.default_rng(3).permutation(len(X))).cuda()
    yp, ip, dp = ix.retrieve(Xd[perm].contiguous(), k=8, ratio=0.5, return_neighbours=True, nprobe=4)
    assert torch.equal(ip, idx[perm]) and torch.equal(bits(dp), bits(dist[perm])) and torch.equal(bits(yp), bits(y[perm]))
    assert torch.equal(bits(ix.search(Xd[perm].contiguous(), k=8, nprobe=4)[1]), bits(s_sc[perm]))
    for n in (0, 1, 63, 64, 127, 128, 256):
        y1, i1, d1 = ix.retrieve(Xd[n:n + 1].contiguous(), k=8, ratio=0.5, return_neighbours=True, nprobe=4)
        assert torch.equal(i1[0], idx[n]) and torch.equal(bits(d1[0]), bits(dist[n])) and torch.equal(bits(y1[0]), bits(y[n])), n


# ---- hygiene ----
def test_repeat_with_garbage_in_the_workspace():
    from lds import native
    X, P, ix, ivf = gaussian()
    Xd = dev(X)
    pool, h = ix._device(Xd.device)
    on = ix._device_ivf(Xd.device)
    ws = torch.empty(native.ivf_workspace_bytes(len(X), len(P), X.shape[1], 8, ix.nlist, 4), dtype=torch.uint8, device="cuda")
    outs = []
    for fill in (NAN_WORD, X7F_WORD, NAN_WORD):
        native.debug_fill(ws, fill)
        outs.append(native.ivf_retrieve(Xd, pool, h, 8, 0.5, on, 4, ws=ws))
        native.debug_fill(ws, fill)
        outs.append(native.ivf_search(Xd, pool, h, 8, on, 4, ws=ws))
    for a in outs[2::2]:
        assert all(torch.equal(bits(u), bits(v)) for u, v in zip(a, outs[0]))
    for a in outs[3::2]:
        assert all(torch.equal(bits(u), bits(v)) for u, v in zip(a, outs[1]))
    assert torch.isfinite(outs[0][0]).all() and torch.equal(outs[0][1], outs[1][0])


def test_nan_query_row_as_in_the_exact_search():
    X, P, ix, ivf = gaussian()
    Xn = np.array(X[:40])
    Xn[7] = np.nan
    Xd = dev(Xn)
    for nprobe in (None, 2):
        idx, sc = ix.search(Xd, k=8, nprobe=nprobe)
        y, ri, _ = ix.retrieve(Xd, k=8, ratio=0.5, return_neighbours=True, nprobe=nprobe)
        assert (idx[7] == -1).all() and (ri[7] == -1).all() and torch.isnan(y[7]).all() and torch.isneginf(sc[7]).all()
        keep = [n for n in range(40) if n != 7]
        assert (idx[keep] >= 0).all() and torch.isfinite(y[keep]).all()
    assert (ix.probe_lists(Xd, 2)[7] == -1).all()
    assert torch.equal(ix.search(Xd, k=8, nprobe=2)[0][keep], ix.search(dev(X[:40]), k=8, nprobe=2)[0][keep])


def test_ragged_form():
    X, P, ix, ivf = gaussian()
    B, T, lengths = 3, 40, (40, 0, 17)
    Xr = np.full((B, T, X.shape[1]), np.nan, np.float32)
    Xr[0], Xr[2, :17] = X[:40], X[40:57]
    y, idx, dist = ix.retrieve(dev(Xr), k=8, ratio=0.5, lengths=lengths, return_neighbours=True, nprobe=4)
    yd, id_, dd = ix.retrieve(dev(X[:57]), k=8, ratio=0.5, return_neighbours=True, nprobe=4)
    assert y.shape == (B, T, X.shape[1]) and idx.shape == dist.shape == (B, T, 8)
    for got, want in ((y, yd), (dist, dd)):
        assert torch.equal(bits(got[0]), bits(want[:40])) and torch.equal(bits(got[2, :17]), bits(want[40:]))
        assert not got[1].any() and not got[2, 17:].any()
    assert torch.equal(idx[0], id_[:40]) and torch.equal(idx[2, :17], id_[40:]) and (idx[1] == -1).all() and (idx[2, 17:] == -1).all()


def _raw(ix, X, k, nprobe, **over):
    """lds_ivf_search through the raw binding with single tables replaced"""
    from lds import native
    Xd = dev(X)
    pool, h = ix._device(Xd.device)
    names = ("centres", "hc", "offsets", "order", "copy", "hl")
    on = tuple(over.get(n, t) for n, t in zip(names, ix._device_ivf(Xd.device)))
    idx, sc = native.ivf_search(Xd, pool, h, k, on, nprobe)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), sc.cpu().numpy()


def test_corrupt_tables_lead_nowhere():
    """offsets that decrease, do not start at 0, do not end at M or do not pad to the copy's rows (the first list 60 rows longer at the second's
    cost: one block more): every query comes back with -1 everywhere;
    `order` values outside the pool are clamped into it (the scores stay the lists' own)"""
    case = IV.LATTICE[5]
    N, M, D, k, L, nprobe = case
    X, P, ix, ivf = lattice(case)
    good_idx, good_sc = _raw(ix, X, k, nprobe)
    off = ivf[1]
    bad = {"decreasing": np.concatenate([off[:2], off[1:2] - 1, off[3:]]), "start": np.concatenate([[1], off[1:]]),
           "end": np.concatenate([off[:-1], [M + 5]]), "huge": np.concatenate([off[:1], [2 ** 40], off[2:]]),
           "negative": np.concatenate([off[:1], [-7], off[2:]]), "other_padding": np.concatenate([off[:1], off[1:2] + 60, off[2:]])}
    for name, o in bad.items():
        assert o.shape == off.shape and not np.array_equal(o, off), name
        idx, sc = _raw(ix, X, k, nprobe, offsets=dev(o.astype(np.int64)))
        assert (idx == -1).all() and np.isneginf(sc).all(), name
    wild = np.array(ivf[2])
    wild[::3], wild[1::3] = 2 ** 31 - 1, -5
    idx, sc = _raw(ix, X, k, nprobe, order=dev(wild))
    assert idx.min() >= 0 and idx.max() < M and np.array_equal(sc, good_sc)
    again = _raw(ix, X, k, nprobe)
    assert np.array_equal(again[0], good_idx) and np.array_equal(again[1], good_sc)


def test_limits_return_codes_and_enqueue_nothing():
    from lds import native
    L = native.lib()
    case = IV.LATTICE[5]
    N, M, D, k, nc, nprobe = case
    X, P, ix, ivf = lattice(case)
    Xd = dev(X)
    pool, h = ix._device(Xd.device)
    on = ix._device_ivf(Xd.device)
    nlist, rows = ix.nlist, on[4].shape[0]
    need = native.ivf_workspace_bytes(N, M, D, k, nlist, nprobe)
    big = torch.zeros(N * D + 4, device="cuda")

    def call(entry="retrieve", N=N, M=M, D=D, k=k, nlist=nlist, nprobe=nprobe, rows=rows, ratio=0.5, ws_bytes=need, x=Xd, null=None, lengths=None, B=1, T=N):
        y = torch.full((N, D), 7.0, device="cuda")
        idx = torch.full((N, 8), 7, dtype=torch.int32, device="cuda")
        dist = torch.full((N, 8), 7.0, device="cuda")
        ws = torch.zeros(max(ws_bytes, 16), dtype=torch.uint8, device="cuda")
        t = {n: v.data_ptr() for n, v in zip(("centres", "hc", "offsets", "order", "copy", "hl"), on)}
        if null:
            t[null] = None
        index = (t["centres"], t["hc"], nlist, t["offsets"], t["order"], t["copy"], t["hl"], rows, nprobe)
        tail = (idx.data_ptr(), dist.data_ptr(), ws.data_ptr(), ws_bytes, native._stream())
        if entry == "search":
            rc = L.lds_ivf_search(x.data_ptr(), N, pool.data_ptr(), h.data_ptr(), M, D, k, *index, *tail)
        elif entry == "forced":
            rc = L.lds_test_ivf_search(x.data_ptr(), N, pool.data_ptr(), h.data_ptr(), M, D, k, *index, 128, *tail)
        elif entry == "ragged":
            ln = (ct.c_int32 * B)(*lengths)
            rc = L.lds_ivf_retrieve_ragged(x.data_ptr(), B, T, ct.cast(ln, ct.c_void_p), pool.data_ptr(), h.data_ptr(), M, D, k, *index, ratio, y.data_ptr(), *tail)
        else:
            rc = L.lds_ivf_retrieve(x.data_ptr(), N, pool.data_ptr(), h.data_ptr(), M, D, k, *index, ratio, y.data_ptr(), *tail)
        torch.cuda.synchronize()
        assert bool((y == 7).all()) and bool((idx == 7).all()) and bool((dist == 7).all()) and not bool(ws.any()), "something ran"
        return rc

    err = L.lds_last_error
    for entry in ("retrieve", "search", "forced"):
        assert call(entry, D=12) == -1 and b"D 12" in err()
        assert call(entry, k=9) == -1 and b"k 9" in err()
        assert call(entry, k=0) == -1 and b"k 0" in err()
        assert call(entry, M=16777217) == -1 and b"M 16777217" in err()
        assert call(entry, N=0) == -1 and b"N 0" in err()
        assert call(entry, nprobe=0) == -1 and b"nprobe 0" in err()
        assert call(entry, nprobe=9) == -1 and b"nprobe 9" in err()
        assert call(entry, nlist=2, nprobe=3) == -1 and b"nprobe 3" in err()
        assert call(entry, nlist=0) == -1 and b"nlist 0" in err()
        assert call(entry, nlist=65537) == -1 and b"nlist 65537" in err()
        assert call(entry, nlist=M + 1) == -1 and b"nlist" in err()
        assert call(entry, rows=rows + 1) == -1 and b"copy_rows" in err()
        assert call(entry, rows=M - M % 128) == -1 and b"copy_rows" in err()
        assert call(entry, rows=(M + 127 * nlist) // 128 * 128 + 128) == -1 and b"copy_rows" in err()
        assert call(entry, x=big[1:1 + N * D]) == -1 and b"aligned" in err()
        for table in ("centres", "hc", "offsets", "order", "copy", "hl"):
            assert call(entry, null=table) == -1 and b"null" in err()
        assert call(entry, ws_bytes=need - 256) == -2 and str(need).encode() in err()
    for ratio in (-0.5, 1.5, float("nan")):
        assert call(ratio=ratio) == -1 and b"ratio" in err()
        assert call("ragged", ratio=ratio, lengths=[N]) == -1 and b"ratio" in err()
    assert call("ragged", lengths=[N + 1]) == -1 and b"lengths[0]" in err()
    assert call("ragged", B=65, T=1, lengths=[1] * 65) == -1 and b"B 65" in err()
    assert call("ragged", lengths=[N], ws_bytes=need - 256) == -2
    # and the same call inside the limits runs
    assert np.array_equal(ix.search(Xd, k=k, nprobe=nprobe)[0].cpu().numpy(), IV.search(X, P, k, ivf, nprobe)[0])


# ---- the pipeline ----
def test_infer_from_long_audio_with_an_ivf_index():
    import infer_svc
    import test_gpu_knn as TK
    from cluster.index import UnitsIndex
    from tools.slicer import split_ranges
    svc = infer_svc.synthetic_svc("cuda", width=64, layers=1)
    sr = 22050
    audio = dev(infer_svc.synthetic_recording(6.0, sr))
    pool = np.random.default_rng(4).standard_normal((300, 64)).astype(np.float32)
    ix = UnitsIndex(pool).build_ivf(6, centres=IV.gaussian_centres(6, 64))
    ranges = split_ranges(audio, sr, 512 * sr / 44100, db_thresh=-40, min_len=500)
    n_frames = svc._plan_long_audio(sr, ranges, 16)["n_frames"]
    g = torch.Generator(device="cuda").manual_seed(5)
    x_T = [torch.randn((1, 1, svc.model.decoder.out_dims, n), device="cuda", generator=g) for n in n_frames]
    want, _ = TK.by_hand(svc, audio, sr, x_T, lambda u, f: ix.retrieve(u, k=8, ratio=0.5, lengths=f, nprobe=2))
    got, rate = svc.infer_from_long_audio(audio, sr=sr, x_T=x_T, index=ix, index_ratio=0.5, index_nprobe=2, **TK.KW)
    assert rate == 44100 and torch.isfinite(got).all() and torch.equal(bits(got), bits(want))
    exact, _ = svc.infer_from_long_audio(audio, sr=sr, x_T=x_T, index=ix, index_ratio=0.5, **TK.KW)
    assert exact.shape == got.shape and not torch.equal(exact, got)      # (two of six lists: other neighbours than the exact search's)
    with pytest.raises(ValueError, match="nprobe must be"):
        svc.infer_from_long_audio(audio, sr=sr, x_T=x_T, index=ix, index_nprobe=9, **TK.KW)
    with pytest.raises(ValueError, match="needs an IVF"):
        svc.infer_from_long_audio(audio, sr=sr, x_T=x_T, index=UnitsIndex(pool), index_nprobe=2, **TK.KW)


def test_infer_svc_takes_index_nprobe(tmp_path):
    import infer_svc
    from cluster.index import UnitsIndex
    pool = np.random.default_rng(6).standard_normal((200, 64)).astype(np.float32)
    UnitsIndex(pool).build_ivf(5, centres=IV.gaussian_centres(5, 64)).save(tmp_path / "ivf_index.pt")
    assert UnitsIndex.load(tmp_path / "ivf_index.pt").nlist == 5
    args = ["--synthetic", "--synthetic_width", "64", "--synthetic_layers", "1", "--synthetic_seconds", "4", "-sr", "22050", "-s", "250", "--min_len", "500",
            "--index", str(tmp_path / "ivf_index.pt"), "--index_ratio", "0.75", "--index_k", "4"]
    a = infer_svc.main(args + ["-o", str(tmp_path / "a.npy"), "--index_nprobe", "1"])
    b = infer_svc.main(args + ["-o", str(tmp_path / "b.npy")])
    assert a.shape == b.shape and np.isfinite(a).all() and np.abs(a).max() > 0 and not np.array_equal(a, b)
