"""Units retrieval on a real MI355X (csrc/knn.hip through lds.native, cluster.index.UnitsIndex, DiffusionSVC.infer_from_long_audio and the
two command-line tools) against the float64 oracle of tests/knn_numpy.py: exact index lists on lattice inputs (slabs, splits, short splits,
triplicated pools), the a-priori distance bound on Gaussian inputs, the blend on the GPU's own neighbours, bit-for-bit invariances, the
limits, and the pipeline."""
import ctypes as ct
import functools

import numpy as np
import pytest

import knn_numpy as KN

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NAN_WORD, X7F_WORD = 0x7FC00000, 0x7F7F7F7F


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()      # (a copy: the shared inputs are read-only)


def bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def gaussian(case):
    """(X, P, the oracle's idx, its distances): computed once, shared, never written to"""
    N, M, D, k = case
    X, P = KN.gaussian_case(N, M, D)
    idx, _ = KN.search64(X, P, k)
    out = (X, P, idx, KN.dist64(X, P, idx))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def gaussian_index(case):
    from cluster.index import UnitsIndex
    return UnitsIndex(np.array(gaussian(case)[1]))      # (a copy: the shared pool is read-only)


def forced_search(X, P, k, slab_rows, splits, fill=None):
    """lds_test_knn_search: the pool cut into slabs of slab_rows and `splits` ranges of pool blocks"""
    from lds import native
    Pd = dev(P)
    ws = torch.empty(2 * (splits * len(X) * 8 * 4 + 256), dtype=torch.uint8, device="cuda")
    if fill is not None:
        native.debug_fill(ws, fill)
    return native.knn_search(dev(X), Pd, native.knn_prepare(Pd), k, ws=ws, slab_rows=slab_rows, splits=splits)


# ---- lattice cases: every score exact in fp32, so the index lists are the oracle's, rank by rank ----
@pytest.mark.parametrize("case", KN.LATTICE, ids=lambda c: "x".join(map(str, c)))
def test_lattice_exact(case):
    from cluster.index import UnitsIndex
    N, M, D, k = case
    X, P = KN.lattice_case(N, M, D)
    want, score = KN.search64(X, P, k)
    idx, sc = UnitsIndex(P).search(dev(X), k=k)
    assert idx.dtype == torch.int64 and idx.shape == (N, k) and np.array_equal(idx.cpu().numpy(), want)
    assert np.array_equal(sc.cpu().numpy().astype(np.float64), score)      # (exact: integers and halves)
    y, ri, _ = UnitsIndex(P).retrieve(dev(X), k=k, ratio=0.5, return_neighbours=True)
    assert np.array_equal(ri.cpu().numpy(), want)


@pytest.mark.parametrize("splits", [1, 2, 3])
@pytest.mark.parametrize("M", [333, 261])      # three pool blocks of 128, 128 and 77 or 5 rows: with 3 splits the last holds fewer than k = 8 rows
def test_lattice_slabs_and_splits(M, splits):
    X, P = KN.lattice_case(129, M, 8)
    want, score = KN.search64(X, P, 8)
    idx, sc = forced_search(X, P, 8, 128, splits, fill=NAN_WORD)
    assert np.array_equal(idx.cpu().numpy(), want) and np.array_equal(sc.cpu().numpy().astype(np.float64), score)


@pytest.mark.parametrize("how", ["library", "slabs_128_splits_3", "slabs_256_splits_2"])
def test_lattice_triplicated_pool(how):
    """every pool row appears three times, 100 rows apart: the copies tie exactly and come lowest index first, across blocks, slabs and splits"""
    from cluster.index import UnitsIndex
    X, P = KN.lattice_case(130, 100, 24)
    P3 = np.concatenate([P, P, P])
    want, _ = KN.search64(X, P3, 8)
    if how == "library":
        idx = UnitsIndex(P3).search(dev(X), k=8)[0]
    else:
        idx = forced_search(X, P3, 8, int(how.split("_")[1]), int(how.split("_")[3]))[0]
    assert np.array_equal(idx.cpu().numpy(), want)
    assert (want[:, 0] < 100).all() and (np.diff(want[:, :3], axis=1) > 0).all()      # (the oracle itself: the winner's copies in index order)


# ---- Gaussian cases: the a-priori bound ----
@pytest.mark.parametrize("case", KN.GAUSSIAN, ids=lambda c: "x".join(map(str, c)))
def test_gaussian_within_search_bound(case, record_margin):
    """every returned neighbour's true (float64) distance equals the oracle's distance of the same rank within E_n (knn_numpy.search_bound);
    indices distinct and inside [0, M); rows whose list differs from the oracle's at all: at most 2 % (tests/test_cpu_knn.py: fp32 itself stays
    under 0.5 % on these inputs)"""
    N, M, D, k = case
    X, P, want, d_want = gaussian(case)
    idx, score = gaussian_index(case).search(dev(X), k=k)
    idx = idx.cpu().numpy()
    assert idx.min() >= 0 and idx.max() < M and all(len(set(r)) == k for r in idx)
    E = KN.search_bound(X, P)
    worst = float((np.abs(KN.dist64(X, P, idx) - d_want) / E[:, None]).max())
    differing = int((idx != want).any(1).sum())
    print(f"{case}: worst distance error / E_n {worst:.3g}; rows whose list differs from float64's: {differing} of {N}")
    record_margin(worst, 1.0)
    assert differing <= 0.02 * N
    x2 = (X.astype(np.float64) ** 2).sum(1)[:, None]
    assert (np.abs(x2 - 2 * score.cpu().numpy() - KN.dist64(X, P, idx)) <= E[:, None]).all()      # the scores are the winners' own


# ---- blend: against the oracle evaluated on the GPU's own neighbours ----
@pytest.mark.parametrize("k,ratio", [(8, 0.5), (4, 0.25), (1, 0.75), (3, 1.0)])
def test_blend_on_own_neighbours(k, ratio, record_margin):
    case = KN.GAUSSIAN[0]
    X, P = gaussian(case)[:2]
    D = X.shape[1]
    y, idx, dist = gaussian_index(case).retrieve(dev(X), k=k, ratio=ratio, return_neighbours=True)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy().astype(np.float64)
    y64, d64, w64 = KN.blend64(X, P, idx, ratio)
    bound = KN.blend_bound(X, P)
    worst = float(np.abs(y.cpu().numpy() - y64).max() / bound)
    print(f"k {k} ratio {ratio}: |y - y64| / bound {worst:.3g}")
    record_margin(worst, 1.0)
    # a sum of D squares of differences: (D + 4) 2^-24 relative; the normalised weights carry twice that twice over (square, normalisation)
    assert (np.abs(dist - d64) <= (D + 4) * 2.0 ** -24 * d64).all()
    assert (np.abs(KN.weights64(dist) - w64) <= 4 * (D + 4) * 2.0 ** -24).all()


def test_blend_exact_ends_and_pool_rows():
    case = KN.GAUSSIAN[0]
    X, P = gaussian(case)[:2]
    ix, Xd = gaussian_index(case), dev(X)
    y0, i0, _ = ix.retrieve(Xd, k=8, ratio=0.0, return_neighbours=True)
    assert torch.equal(bits(y0), bits(Xd))                                   # ratio 0: x bit for bit (the search still ran)
    assert np.array_equal(i0.cpu().numpy(), ix.search(Xd, k=8)[0].cpu().numpy())
    y1, i1, _ = ix.retrieve(Xd, k=1, ratio=1.0, return_neighbours=True)
    assert torch.equal(bits(y1), bits(dev(P)[i1[:, 0]]))                     # ratio 1, k 1: the pool row bit for bit
    rows = np.array([0, 127, 128, 2500, 4999])
    yq, iq, dq = ix.retrieve(dev(P[rows]), k=8, ratio=1.0, return_neighbours=True)
    assert np.array_equal(iq[:, 0].cpu().numpy(), rows) and (dq[:, 0] == float(np.float32(KN.FLOOR))).all() and (dq[:, 1:] > 1).all()
    assert (np.abs(yq.cpu().numpy() - P[rows].astype(np.float64)) <= KN.blend_bound(P[rows], P)).all()      # d = 0 takes the floor: that row


# ---- as if alone, repeat, garbage in the workspace ----
def test_row_as_if_alone():
    """row n of an N = 129 call = the N = 1 call on that row, bit for bit in idx, dist and y; and the scores do not depend on the split"""
    case = KN.GAUSSIAN[0]
    X, P = gaussian(case)[:2]
    ix, Xd = gaussian_index(case), dev(X[:129])
    y, idx, dist = ix.retrieve(Xd, k=8, ratio=0.5, return_neighbours=True)
    for n in (0, 1, 31, 32, 63, 64, 100, 127, 128):
        y1, i1, d1 = ix.retrieve(Xd[n:n + 1].contiguous(), k=8, ratio=0.5, return_neighbours=True)
        assert torch.equal(i1[0], idx[n]) and torch.equal(bits(d1[0]), bits(dist[n])) and torch.equal(bits(y1[0]), bits(y[n])), n
    yb, ib, db = ix.retrieve(dev(np.concatenate([X[200:257], X[:129]])), k=8, ratio=0.5, return_neighbours=True)      # other rows in front
    assert torch.equal(ib[57:], idx) and torch.equal(bits(db[57:]), bits(dist)) and torch.equal(bits(yb[57:]), bits(y))
    base = forced_search(X[:129], P, 8, 4992, 1)
    for slab_rows, splits in ((128, 7), (1024, 40), (2560, 2)):
        got = forced_search(X[:129], P, 8, slab_rows, splits)
        assert torch.equal(got[0], base[0]) and torch.equal(bits(got[1]), bits(base[1])), (slab_rows, splits)
    assert torch.equal(base[0].to(torch.int64), idx)


def test_repeat_with_garbage_in_the_workspace():
    from lds import native
    case = KN.GAUSSIAN[0]
    X, P = gaussian(case)[:2]
    Xd = dev(X)
    pool, h = gaussian_index(case)._device(Xd.device)
    ws = torch.empty(native.knn_workspace_bytes(len(X), len(P), X.shape[1], 8), dtype=torch.uint8, device="cuda")
    outs = []
    for fill in (NAN_WORD, X7F_WORD, NAN_WORD):
        native.debug_fill(ws, fill)
        outs.append(native.knn_retrieve(Xd, pool, h, 8, 0.5, ws=ws))
        native.debug_fill(ws, fill)
        outs.append(native.knn_search(Xd, pool, h, 8, ws=ws))
    for a in outs[2::2]:
        assert all(torch.equal(bits(u), bits(v)) for u, v in zip(a, outs[0]))
    for a in outs[3::2]:
        assert all(torch.equal(bits(u), bits(v)) for u, v in zip(a, outs[1]))
    assert torch.isfinite(outs[0][0]).all() and torch.equal(outs[0][1], outs[1][0])


def test_ragged_form():
    case = KN.GAUSSIAN[0]
    X, P = gaussian(case)[:2]
    ix = gaussian_index(case)
    B, T, lengths = 3, 40, (40, 0, 17)
    Xr = np.full((B, T, X.shape[1]), np.nan, np.float32)
    Xr[0], Xr[2, :17] = X[:40], X[40:57]
    y, idx, dist = ix.retrieve(dev(Xr), k=8, ratio=0.5, lengths=lengths, return_neighbours=True)
    yd, id_, dd = ix.retrieve(dev(X[:57]), k=8, ratio=0.5, return_neighbours=True)
    assert y.shape == (B, T, X.shape[1]) and idx.shape == dist.shape == (B, T, 8)
    for got, want in ((y, yd), (dist, dd)):
        assert torch.equal(bits(got[0]), bits(want[:40])) and torch.equal(bits(got[2, :17]), bits(want[40:]))
        assert not got[1].any() and not got[2, 17:].any()
    assert torch.equal(idx[0], id_[:40]) and torch.equal(idx[2, :17], id_[40:]) and (idx[1] == -1).all() and (idx[2, 17:] == -1).all()
    assert torch.equal(bits(ix.retrieve(dev(Xr), k=8, ratio=0.5, lengths=torch.tensor(lengths))), bits(y))


# ---- every limit returns its code and enqueues nothing ----
def test_limits_return_codes_and_enqueue_nothing():
    from lds import native
    L = native.lib()
    N, M, D, k = 37, 300, 16, 4
    X, P = KN.lattice_case(N, M, D)
    Xd, Pd = dev(X), dev(P)
    h = native.knn_prepare(Pd)
    need = native.knn_workspace_bytes(N, M, D, k)
    big = torch.zeros(N * 24 + 4, device="cuda")      # room for a misaligned X of width 24

    def call(entry="retrieve", N=N, M=M, D=D, k=k, ratio=0.5, ws_bytes=need, x=Xd, null_y=False, lengths=None, B=1, T=N):
        y = torch.full((N, 24), 7.0, device="cuda")
        idx = torch.full((N, 8), 7, dtype=torch.int32, device="cuda")
        dist = torch.full((N, 8), 7.0, device="cuda")
        ws = torch.zeros(max(ws_bytes, 16), dtype=torch.uint8, device="cuda")
        tail = (idx.data_ptr(), dist.data_ptr(), ws.data_ptr(), ws_bytes, native._stream())
        if entry == "search":
            rc = L.lds_knn_search(x.data_ptr(), N, Pd.data_ptr(), h.data_ptr(), M, D, k, *tail)
        elif entry == "forced":
            rc = L.lds_test_knn_search(x.data_ptr(), N, Pd.data_ptr(), h.data_ptr(), M, D, k, 128, 2, *tail)
        elif entry == "ragged":
            ln = (ct.c_int32 * B)(*lengths)
            rc = L.lds_knn_retrieve_ragged(x.data_ptr(), B, T, ct.cast(ln, ct.c_void_p), Pd.data_ptr(), h.data_ptr(), M, D, k, ratio, y.data_ptr(), *tail)
        else:
            rc = L.lds_knn_retrieve(x.data_ptr(), N, Pd.data_ptr(), h.data_ptr(), M, D, k, ratio, None if null_y else y.data_ptr(), *tail)
        torch.cuda.synchronize()
        assert bool((y == 7).all()) and bool((idx == 7).all()) and bool((dist == 7).all()) and not bool(ws.any()), "something ran"
        return rc

    err = L.lds_last_error
    for entry in ("retrieve", "search", "forced"):
        assert call(entry, D=12) == -1 and b"D 12" in err()
        assert call(entry, k=9) == -1 and b"k 9" in err()
        assert call(entry, k=0) == -1 and b"k 0" in err()
        assert call(entry, M=3) == -1 and b"k 4" in err()
        assert call(entry, M=16777217) == -1 and b"M 16777217" in err()
        assert call(entry, N=0) == -1 and b"N 0" in err()
        assert call(entry, x=big[1:1 + N * D]) == -1 and b"aligned" in err()
        assert call(entry, ws_bytes=need - 256 if entry != "forced" else 256) == -2 and b"workspace" in err()
    for ratio in (-0.5, 1.5, float("nan")):
        assert call(ratio=ratio) == -1 and b"ratio" in err()
        assert call("ragged", ratio=ratio, lengths=[N]) == -1 and b"ratio" in err()
    assert call(null_y=True) == -1 and b"null" in err()
    assert call("ragged", lengths=[N + 1]) == -1 and b"lengths[0]" in err()
    assert call("ragged", lengths=[-1]) == -1 and b"lengths[0]" in err()
    assert call("ragged", B=65, T=1, lengths=[1] * 65) == -1 and b"B 65" in err()
    assert call("ragged", lengths=[N], ws_bytes=need - 256) == -2
    # and the same calls inside the limits run
    Xp = dev(np.concatenate([X, np.zeros((N, 8), np.float32)], 1))      # (the helper's y is 24 wide: a pool of that width)
    Pp = np.concatenate([P, np.zeros((M, 8), np.float32)], 1)
    from cluster.index import UnitsIndex
    assert np.array_equal(UnitsIndex(Pp).retrieve(Xp, k=k, return_neighbours=True)[1].cpu().numpy(), KN.search64(X, P, k)[0])


# ---- the pipeline ----
SPEEDUP = 250      # 1000 // 250 = 4 sampler steps
KW = dict(infer_speedup=SPEEDUP, method="unipc", threhold=-60, threhold_for_split=-40, min_len=500)


@pytest.fixture(scope="module")
def svc():
    import infer_svc
    return infer_svc.synthetic_svc("cuda", width=64, layers=1)


def by_hand(svc, audio, sr, x_T, between, batch_size=16):
    """the stages of DiffusionSVC.infer_from_long_audio one by one, with `between(units, unit_frames)` after the encoder"""
    from lds import native
    from tools.slicer import split_ranges
    from tools.tools import units_forced_alignment_ragged
    rate, block = svc.args["data"]["sampling_rate"], svc.args["data"]["block_size"]
    ranges = split_ranges(audio, sr, block * sr / rate, db_thresh=-40, min_len=500)
    plan = svc._plan_long_audio(sr, ranges, batch_size)
    mask = svc.extract_volume_and_mask(audio, sr, threhold=-60.0)[1]
    n_frames, M = plan["n_frames"], svc.model.decoder.out_dims
    wavs = [None] * len(ranges)
    for idx in plan["chunks"]:
        lens = [ranges[s][2] - ranges[s][1] for s in idx]
        batch = torch.zeros(len(idx), max(lens), device="cuda")
        for j, s in enumerate(idx):
            batch[j, :lens[j]] = audio[ranges[s][1]:ranges[s][2]]
        units, unit_frames = svc.units_encoder.encode_ragged(batch, lens, sample_rate=sr, pad_short=True)
        units = between(units, unit_frames)
        nf = [n_frames[s] for s in idx]
        units = units_forced_alignment_ragged(units, unit_frames, nf)
        noise = torch.zeros(len(idx), 1, M, max(nf), device="cuda")
        for j, s in enumerate(idx):
            noise[j, :, :, :nf[j]] = x_T[s][0]
        wav = svc.vocoder.infer_ragged(svc.call_ragged(units, nf, spk_id=1, infer_speedup=SPEEDUP, method="unipc", x_T=noise), nf)
        for j, s in enumerate(idx):
            wavs[s] = wav[j, 0, :nf[j] * block]
    length = [n * block for n in n_frames]
    offset = np.concatenate([[0], np.cumsum(length)[:-1]])
    return native.overlap_assemble(torch.cat(wavs), offset, [r[0] * block for r in ranges], length, mask.reshape(-1)), n_frames


def test_infer_from_long_audio_with_an_index(svc):
    import infer_svc
    from cluster.index import UnitsIndex
    sr = 22050
    audio = dev(infer_svc.synthetic_recording(6.0, sr))
    ix = UnitsIndex(np.random.default_rng(4).standard_normal((300, 64)).astype(np.float32))
    from tools.slicer import split_ranges
    ranges = split_ranges(audio, sr, 512 * sr / 44100, db_thresh=-40, min_len=500)
    n_frames = svc._plan_long_audio(sr, ranges, 16)["n_frames"]
    assert len(ranges) >= 2
    g = torch.Generator(device="cuda").manual_seed(5)
    x_T = [torch.randn((1, 1, svc.model.decoder.out_dims, n), device="cuda", generator=g) for n in n_frames]
    want, _ = by_hand(svc, audio, sr, x_T, lambda u, f: ix.retrieve(u, k=8, ratio=0.5, lengths=f))
    got, rate = svc.infer_from_long_audio(audio, sr=sr, x_T=x_T, index=ix, index_ratio=0.5, **KW)
    assert rate == 44100 and torch.isfinite(got).all() and torch.equal(bits(got), bits(want))
    plain, _ = svc.infer_from_long_audio(audio, sr=sr, x_T=x_T, **KW)
    assert plain.shape == got.shape and not torch.equal(plain, got)
    assert torch.equal(bits(by_hand(svc, audio, sr, x_T, lambda u, f: u)[0]), bits(plain))
    zero, _ = svc.infer_from_long_audio(audio, sr=sr, x_T=x_T, index=ix, index_ratio=0.0, index_k=3, **KW)
    assert torch.equal(bits(zero), bits(plain))
    with pytest.raises(ValueError, match="k must be"):
        svc.infer_from_long_audio(audio, sr=sr, x_T=x_T, index=ix, index_k=9, **KW)


def test_infer_svc_takes_an_index(tmp_path):
    import infer_svc
    from cluster.index import UnitsIndex
    UnitsIndex(np.random.default_rng(6).standard_normal((200, 64)).astype(np.float32)).save(tmp_path / "svc_index.pt")
    args = ["--synthetic", "--synthetic_width", "64", "--synthetic_layers", "1", "--synthetic_seconds", "4", "-sr", "22050", "-s", str(SPEEDUP), "--min_len", "500"]
    a = infer_svc.main(args + ["-o", str(tmp_path / "a.npy"), "--index", str(tmp_path / "svc_index.pt"), "--index_ratio", "0.75", "--index_k", "4"])
    b = infer_svc.main(args + ["-o", str(tmp_path / "b.npy")])
    assert a.shape == b.shape and np.isfinite(a).all() and np.abs(a).max() > 0 and not np.array_equal(a, b)


def test_infer_tts_takes_an_index(tmp_path):
    import infer_tts
    from cluster.index import UnitsIndex
    UnitsIndex(np.random.default_rng(7).uniform(-1.7, 1.7, (64, 1280)).astype(np.float32)).save(tmp_path / "tts_index.pt")
    targs = ["--synthetic", "--synthetic_tokens", "16", "-s", str(SPEEDUP)]
    torch.manual_seed(2)
    c = infer_tts.main(targs + ["-o", str(tmp_path / "c.npy"), "--index", str(tmp_path / "tts_index.pt")])
    torch.manual_seed(2)
    d = infer_tts.main(targs + ["-o", str(tmp_path / "d.npy")])
    assert c.shape == d.shape == (16 * 512,) and np.isfinite(c).all() and not np.array_equal(c, d)
