"""float64 restatement of the cosine metric of the clustering stack (include/lds.h LDS_METRIC_COSINE: lds_kmeans_*_metric, lds_knn_*_metric,
lds_ivf_*_metric) in the pattern of tests/knn_numpy.py and tests/kmeans_numpy.py, with the seeded inputs and the a-priori bounds that
tests/test_cpu_cosine.py and tests/test_gpu_cosine.py share.

  row constant  r(v) = 1 / max(|v|, 1e-12)
  score         (x . p) r(p): what decides the order (descending, the lower index among equal scores); reported: score * r(x) = cos(x, p)
  distance      d = 1/2 sum (x r(x) - p r(p))^2 = 1 - cos, floored at 1e-12
  weights       "inverse_square": (1 / d)^2 normalised; "uniform": 1 / found, over the neighbours present (idx >= 0)
  blend         y = (1 - ratio) x + ratio sum_j w_j p_j over the ORIGINAL rows

Bounds (u = 2^-24, all derived before any kernel ran):
  SIM    a compared similarity is off by at most (D + 4) u: the dot product's chain of D fused multiply-adds contributes D u |x||p|, which
         the two row constants turn into D u; r itself (a sum of non-negative squares, whose relative error the square root halves, the
         square root, the reciprocal) and the product with it the remaining 4 u.  `sim_bound(D)`.
  SEARCH two similarities decide an order, so a returned neighbour's true similarity lies at most 2 (D + 4) u below the oracle's of the
         same rank (and never above it: the oracle's is the best possible).  `search_bound(D)`.
  DIST   d = 1/2 |a - b|^2 with a = x r(x), b = p r(p).  The errors of the two row constants are common factors of a and of b: to first
         order they change d by (e_a a - e_b b) . (a - b) = (e_a + e_b) d, i.e. relatively, by 2 ((D + 1) / 2 + 2) u = (D + 5) u.  The
         roundings of the individual products and differences (3 u per element) do not cancel: they move d by at most |a - b| (|a| + |b|)
         u = 2 sqrt(2 d) u, relatively 2 sqrt(2 / d) u.  The sum of D squares and the halving add (D + 2) u.  Together
         e_d(d) = (2 D + 7 + 2 sqrt(2 / d)) u.  `dist_bound(D, d)`.
  BLEND  knn_numpy.blend_bound's argument repeated for normalised rows: the inverse-square weight doubles the distance's relative error,
         the normalisation doubles it again, so sum_j |dw_j| <= 4 e_d(d_min) + 12 u (reciprocal, square, the sum over k <= 8, the division);
         z is a combination of rows bounded by |P|inf, its chain over k <= 8 rows and the final blend add at most 12 u more:
         |y - y64| <= (4 e_d(d_min) + 24 u) max(|X|inf, |P|inf) = (8 (D + 6.5) + 8 sqrt(2 / d_min)) u max(..), d_min the smallest float64
         distance among the blended neighbours.  Uniform weights carry one rounding instead of 4 e_d, so the same bound covers them.
         `blend_bound(X, P, d_min)`.  Euclidean distances with uniform weights: knn_numpy.blend_bound as it is."""
import numpy as np

import kmeans_numpy as KM
import knn_numpy as KN

U24 = 2.0 ** -24
EPS = 1e-12
FLOOR = 1e-12
GAUSSIAN = KN.GAUSSIAN
LATTICE = ((129, 8, 8, 8), (127, 257, 24, 4), (128, 1000, 64, 8))      # (N, M, D, k)
# scaled blobs: name -> (K, D, N, first seed, B (ragged) or 0, lengths)
BLOBS = {
    "blobs_1000x256": (1000, 256, 3000, 200, 0, None),
    "odd_333x136": (333, 136, 1501, 400, 0, None),
    "ragged_1000x256": (1000, 256, 150, 500, 3, (50, 17, 33)),
}
FIT = dict(K=64, D=96, N=6000, seed=7, tol=1e-2, max_iter=200)


# ---- inputs ----
def lattice_rows(rng, R, D):
    """R rows of n in {1, 4, 16} (n <= D) non-zeros of one magnitude a in {1, 2, 4}, random signs and positions: squared norms 1, 4, 16, 64,
    256 or 1024, so every norm and every row constant is a power of two"""
    out = np.zeros((R, D), np.float32)
    counts = [n for n in (1, 4, 16) if n <= D]
    for r in range(R):
        n = counts[rng.integers(len(counts))]
        a = (1.0, 2.0, 4.0)[rng.integers(3)]
        out[r, rng.choice(D, n, replace=False)] = a * rng.choice([-1.0, 1.0], n)
    return out


def lattice_case(N, M, D, seed=0):
    """(X [N, D], P [M, D]): every dot product is an integer of magnitude <= 256, every r a power of two, so every score and every
    similarity is exact in fp32 and scaled copies of a row tie exactly"""
    rng = np.random.default_rng([seed, N, M, D, 7])
    return lattice_rows(rng, N, D), lattice_rows(rng, M, D)


def gaussian_case(N, M, D, seed=0):
    return KN.gaussian_case(N, M, D, seed)


def scaled_blobs(seed, K, D, N, spread=0.5):
    """kmeans_numpy.make_blobs with every centre row and every data row multiplied by a seeded 2^u, u an integer in -2 .. 2 (exact in fp32):
    cosine labels do not move under the scaling, Euclidean ones do"""
    C, X, lab = KM.make_blobs(seed, K, D, N, spread)
    rng = np.random.default_rng([seed, 11])
    C = (C * np.exp2(rng.integers(-2, 3, K)).astype(np.float32)[:, None]).astype(np.float32)
    X = (X * np.exp2(rng.integers(-2, 3, N)).astype(np.float32)[:, None]).astype(np.float32)
    return C, X, lab


# ---- the definitions ----
def row_const(V, dtype=np.float64):
    V = np.asarray(V, dtype)
    s = (V * V).sum(-1, dtype=dtype)
    return (dtype(1.0) / np.maximum(np.sqrt(s), dtype(EPS))).astype(dtype)


def scores(X, P, dtype=np.float64):
    """(x . p) r(p) in `dtype`: the ordering score"""
    X, P = np.asarray(X, dtype), np.asarray(P, dtype)
    return ((X @ P.T) * row_const(P, dtype)[None, :]).astype(dtype)


def sims(X, P, dtype=np.float64):
    """the reported value: the score times r(x)"""
    return (scores(X, P, dtype) * row_const(X, dtype)[:, None]).astype(dtype)


def search64(X, P, k, chunk=64):
    """(idx int64 [N, k], cosine similarity float64 [N, k]): descending score, the lower index among equal scores"""
    idx, sc = [], []
    rx = row_const(X)
    for r in range(0, len(X), chunk):
        s = scores(X[r:r + chunk], P)
        i = KN.topk_stable(s, k)
        idx.append(i)
        sc.append(np.take_along_axis(s, i, 1) * rx[r:r + chunk, None])
    return np.concatenate(idx), np.concatenate(sc)


def sim64(X, P, idx):
    """the true cosine similarity of GIVEN neighbours [N, k]"""
    X64, P64 = np.asarray(X, np.float64), np.asarray(P, np.float64)
    return np.einsum("nd,nkd->nk", X64 * row_const(X)[:, None], P64[idx] * row_const(P)[idx][:, :, None])


def dist64(X, P, idx):
    """d [N, k] = 1/2 sum_c (x_c r_x - p_c r_p)^2 in float64, no floor (idx = -1 reads row 0: mask it yourself)"""
    X64, P64 = np.asarray(X, np.float64), np.asarray(P, np.float64)
    a = X64 * row_const(X)[:, None]
    j = np.where(idx >= 0, idx, 0)
    b = P64[j] * row_const(P)[j][:, :, None]
    return 0.5 * ((a[:, None, :] - b) ** 2).sum(2)


def weights64(d, found, how):
    if how == "uniform":
        w = np.where(found, 1.0 / np.maximum(found.sum(1, keepdims=True), 1), 0.0)
        return w
    assert how == "inverse_square"
    w = np.where(found, (1.0 / np.maximum(d, FLOOR)) ** 2, 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return w / w.sum(1, keepdims=True)


def blend64(X, P, idx, ratio, how="inverse_square", metric="cosine"):
    """(y [N, D], floored d [N, k] (0 where idx = -1), weights [N, k]) for GIVEN neighbours; idx = -1: not found, weight 0"""
    X64, P64 = np.asarray(X, np.float64), np.asarray(P, np.float64)
    found = idx >= 0
    rows = P64[np.where(found, idx, 0)]
    d = dist64(X, P, idx) if metric == "cosine" else ((X64[:, None, :] - rows) ** 2).sum(2)
    d = np.maximum(d, FLOOR)
    w = weights64(d, found, how)
    return (1.0 - ratio) * X64 + ratio * np.einsum("nk,nkd->nd", w, rows), np.where(found, d, 0.0), w


def retrieve_ragged64(X, lengths, P, k, ratio, how="inverse_square"):
    B, T, D = X.shape
    y, idx, d = np.zeros((B, T, D)), np.full((B, T, k), -1, np.int64), np.zeros((B, T, k))
    for b, n in enumerate(lengths):
        if n:
            idx[b, :n] = search64(X[b, :n], P, k)[0]
            y[b, :n], d[b, :n], _ = blend64(X[b, :n], P, idx[b, :n], ratio, how)
    return y, idx, d


# ---- k-means in cosine mode ----
def assign64(X, C, rows=512):
    """(labels = float64 arg-max of the cosine score, lowest index among ties; best = the winning cosine similarity; gap = best - runner-up)"""
    N = len(X)
    lab, best, gap = np.empty(N, np.int64), np.empty(N), np.empty(N)
    for r0 in range(0, N, rows):
        s = sims(X[r0:r0 + rows], C)
        l = s.argmax(1)
        lab[r0:r0 + len(l)], best[r0:r0 + len(l)] = l, s[np.arange(len(l)), l]
        if s.shape[1] > 1:
            part = np.partition(s, -2, axis=1)
            gap[r0:r0 + len(l)] = part[:, -1] - part[:, -2]
        else:
            gap[r0:r0 + len(l)] = np.inf
    return lab, best, gap


def fit64(X, C0, max_iter, tol):
    """the loop of the reference's kmeans.py:177-202 in cosine mode from a given start: the cosine assignment, then the SAME Lloyd step as
    the Euclidean mode (kmeans_numpy.lloyd_step64) -> dict(labels per iteration, errors, centroids, n_iter, num_points)"""
    C, npnt = np.asarray(C0, np.float64), np.ones(len(C0))
    labels, errors = [], []
    for _ in range(max_iter):
        lab = assign64(X, C)[0]
        C, npnt, err, _ = KM.lloyd_step64(X, lab, C, npnt)
        labels.append(lab)
        errors.append(err)
        if err <= tol:
            break
    return {"labels": labels, "errors": np.array(errors), "centroids": C, "n_iter": len(errors), "num_points": npnt}


# ---- IVF in cosine ----
def ivf_build(P, C, dtype=np.float64):
    """ivf_numpy.build with the cosine score: (the centres left, offsets, order)"""
    labels = np.argmax(scores(P, C, dtype), axis=1)
    counts = np.bincount(labels, minlength=len(C))
    keep = np.flatnonzero(counts)
    return np.asarray(C)[keep], np.concatenate([[0], np.cumsum(counts[keep])]).astype(np.int64), np.argsort(labels, kind="stable").astype(np.int32)


def ivf_probe(X, centres, nprobe, dtype=np.float64):
    return KN.topk_stable(scores(X, centres, dtype), nprobe)


def ivf_search(X, P, k, ivf, nprobe, dtype=np.float64, chunk=64):
    """(idx [N, k], similarity [N, k]): the k best rows of the probed lists; -1 / -inf where they hold fewer than k rows"""
    centres, offsets, order = ivf
    list_of = np.empty(len(P), np.int64)
    list_of[order] = np.repeat(np.arange(len(centres)), np.diff(offsets))
    pl = ivf_probe(X, centres, nprobe, dtype)
    rx = row_const(X, dtype)
    idx, sc = [], []
    for r in range(0, len(X), chunk):
        s = scores(X[r:r + chunk], P, dtype)
        cand = (list_of[None, :, None] == pl[r:r + chunk, None, :]).any(2)
        i = KN.topk_stable(np.where(cand, s, -np.inf), k)
        found = np.take_along_axis(cand, i, 1)
        idx.append(np.where(found, i, -1))
        sc.append(np.where(found, np.take_along_axis(s, i, 1) * rx[r:r + chunk, None], -np.inf))
    return np.concatenate(idx), np.concatenate(sc)


# ---- bounds ----
def sim_bound(D):
    return (D + 4) * U24


def search_bound(D):
    return 2.0 * (D + 4) * U24


def dist_bound(D, d):
    """relative: |d_fp32 - d64| <= dist_bound(D, d64) d64"""
    return (2.0 * D + 7.0 + 2.0 * np.sqrt(2.0 / np.asarray(d, np.float64))) * U24


def blend_bound(X, P, d_min):
    D = X.shape[1]
    return (4.0 * dist_bound(D, d_min) + 24.0 * U24) * max(np.abs(X).max(), np.abs(P).max())
