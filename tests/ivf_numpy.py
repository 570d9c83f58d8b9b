"""Restatement of units retrieval through an IVF coarse index (include/lds.h lds_ivf_*) on top of tests/knn_numpy.py: the lists (every pool row
to its best centre, empty lists dropped, ascending original index inside a list), the probed lists (the exact search over the centres), the
k best candidates with the tie rule on ORIGINAL indices and the -1 / -inf fill, and the blend over the entries found.  `dtype` float64 is the
specification; float32 shows what fp32 arithmetic makes of it (tests/test_cpu_ivf.py)."""
import numpy as np

import knn_numpy as KN


def build(P, C, dtype=np.float64):
    """centres C [L, D] -> (the centres left [nlist, D], offsets int64 [nlist + 1], order int32 [M]): pool row m goes to the centre with the
    best score p.c - |c|^2 / 2, the lower centre among equal scores; centres that receive no row are dropped"""
    labels = np.argmax(KN.scores(P, C, dtype), axis=1)      # (the first maximum: the lower centre)
    counts = np.bincount(labels, minlength=len(C))
    keep = np.flatnonzero(counts)
    offsets = np.concatenate([[0], np.cumsum(counts[keep])]).astype(np.int64)
    return np.asarray(C)[keep], offsets, np.argsort(labels, kind="stable").astype(np.int32)


def probe(X, centres, nprobe, dtype=np.float64):
    """int64 [N, nprobe]: the nprobe best centres of every query, best first, the lower centre among equal scores"""
    return KN.topk_stable(KN.scores(X, centres, dtype), nprobe)


def search(X, P, k, ivf, nprobe, dtype=np.float64, chunk=64):
    """ivf = build(..) -> (idx int64 [N, k], score [N, k]): the k best rows among the probed lists' rows by x.p - |p|^2 / 2, descending, the
    lower original index among equal scores; -1 / -inf where the lists hold fewer than k rows"""
    centres, offsets, order = ivf
    list_of = np.empty(len(P), np.int64)
    list_of[order] = np.repeat(np.arange(len(centres)), np.diff(offsets))
    pl = probe(X, centres, nprobe, dtype)
    idx, sc = [], []
    for r in range(0, len(X), chunk):
        s = KN.scores(X[r:r + chunk], P, dtype)
        cand = (list_of[None, :, None] == pl[r:r + chunk, None, :]).any(2)
        i = KN.topk_stable(np.where(cand, s, -np.inf), k)      # (ascending original index among equal scores; the others sort last)
        found = np.take_along_axis(cand, i, 1)
        idx.append(np.where(found, i, -1))
        sc.append(np.where(found, np.take_along_axis(s, i, 1), -np.inf))
    return np.concatenate(idx), np.concatenate(sc)


def blend64(X, P, idx, ratio):
    """knn_numpy.blend64 with idx = -1 allowed: such entries have weight 0, the weights are normalised over the ones found.
    -> (y, floored d with 0 at the missing entries, weights)"""
    X64, P64 = X.astype(np.float64), P.astype(np.float64)
    found = idx >= 0
    rows = P64[np.where(found, idx, 0)]
    d = np.maximum(((X64[:, None, :] - rows) ** 2).sum(2), KN.FLOOR)
    w = np.where(found, (1.0 / d) ** 2, 0.0)
    w = w / w.sum(1, keepdims=True)
    return (1.0 - ratio) * X64 + ratio * np.einsum("nk,nkd->nd", w, rows), np.where(found, d, 0.0), w


def retrieve64(X, P, k, ratio, ivf, nprobe):
    idx, _ = search(X, P, k, ivf, nprobe)
    y, d, _ = blend64(X, P, idx, ratio)
    return y, idx, d


def lattice_centres(L, D, seed=0):
    """integer centres in -3 .. 3 (as knn_numpy.lattice_case): every coarse score is exact in fp32 too"""
    return np.random.default_rng([seed, L, D, 2]).integers(-3, 4, (L, D)).astype(np.float32)


def gaussian_centres(L, D, seed=0):
    return np.random.default_rng([seed, L, D, 3]).standard_normal((L, D)).astype(np.float32)


# (N, M, D, k, centres, nprobe): the lattice cases of tests/test_gpu_ivf.py
LATTICE = ((1, 1, 8, 1, 1, 1), (129, 8, 8, 8, 3, 1), (127, 257, 24, 4, 5, 2), (128, 1000, 64, 8, 2, 2), (128, 1000, 64, 8, 16, 8), (300, 333, 40, 2, 7, 3))
GAUSSIAN_CENTRES = 16      # on KN.GAUSSIAN[0], at nprobe 1 and 4
GAUSSIAN_NPROBE = (1, 4)
