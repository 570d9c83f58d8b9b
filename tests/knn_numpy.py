"""float64 restatement of units retrieval (include/lds.h lds_knn_*): brute-force search with the stable tie rule, the directly recomputed
distances with their floor, the inverse-square weights, the blend and the ragged form -- plus the seeded inputs that the CPU and GPU tests
share (tests/test_cpu_knn.py shows on them what fp32 arithmetic can attain, tests/test_gpu_knn.py holds the kernels to it)."""
import numpy as np

FLOOR = 1e-12
GAUSSIAN = ((257, 5000, 64, 8), (64, 70000, 256, 8))      # (N, M, D, k); the second has M above lds_kmeans_assign's 65,536 centres
LATTICE = ((1, 1, 8, 1), (129, 8, 8, 8), (127, 257, 24, 4), (128, 1000, 64, 8), (300, 333, 40, 2))


def lattice_case(N, M, D, seed=0):
    """integers in -3 .. 3: every score is exact in fp32 (|x.p| <= 9 D, h a multiple of 1/2) and ties are exact"""
    rng = np.random.default_rng([seed, N, M, D])
    return rng.integers(-3, 4, (N, D)).astype(np.float32), rng.integers(-3, 4, (M, D)).astype(np.float32)


def gaussian_case(N, M, D, seed=0):
    rng = np.random.default_rng([seed, N, M, D, 1])
    return rng.standard_normal((N, D)).astype(np.float32), rng.standard_normal((M, D)).astype(np.float32)


def topk_stable(s, k):
    """s [N, M] scores -> idx [N, k] in descending score order, the lower index first among equal scores"""
    return np.argsort(-s, axis=1, kind="stable")[:, :k]


def scores(X, P, dtype=np.float64):
    """x . p - |p|^2 / 2 evaluated in `dtype` (float64: the oracle; float32: what fp32 arithmetic makes of it)"""
    X, P = np.asarray(X, dtype), np.asarray(P, dtype)
    return X @ P.T - (0.5 * (P * P).sum(1, dtype=dtype)).astype(dtype)[None, :]


def search64(X, P, k, chunk=64):
    """(idx int64 [N, k], score float64 [N, k])"""
    idx, sc = [], []
    for r in range(0, len(X), chunk):
        s = scores(X[r:r + chunk], P)
        i = topk_stable(s, k)
        idx.append(i)
        sc.append(np.take_along_axis(s, i, 1))
    return np.concatenate(idx), np.concatenate(sc)


def dist64(X, P, idx):
    """d [N, k] = sum_c (x_c - p_{idx, c})^2 in float64, no floor"""
    X, P = X.astype(np.float64), P.astype(np.float64)
    return np.stack([((X - P[idx[:, j]]) ** 2).sum(1) for j in range(idx.shape[1])], 1)


def weights64(d):
    w = (1.0 / np.maximum(d, FLOOR)) ** 2
    return w / w.sum(1, keepdims=True)


def blend64(X, P, idx, ratio):
    """(y [N, D], floored d [N, k], normalised weights [N, k]) for GIVEN neighbours idx"""
    d = np.maximum(dist64(X, P, idx), FLOOR)
    w = weights64(d)
    z = np.einsum("nk,nkd->nd", w, P.astype(np.float64)[idx])
    return (1.0 - ratio) * X.astype(np.float64) + ratio * z, d, w


def retrieve64(X, P, k, ratio):
    idx, _ = search64(X, P, k)
    y, d, _ = blend64(X, P, idx, ratio)
    return y, idx, d


def retrieve_ragged64(X, lengths, P, k, ratio):
    """X [B, T, D]: rows at and beyond a clip's length give y = 0, idx = -1, dist = 0 whatever they hold"""
    B, T, D = X.shape
    y, idx, d = np.zeros((B, T, D)), np.full((B, T, k), -1, np.int64), np.zeros((B, T, k))
    for b, n in enumerate(lengths):
        if n:
            y[b, :n], idx[b, :n], d[b, :n] = retrieve64(X[b, :n], P, k, ratio)
    return y, idx, d


def search_bound(X, P):
    """E_n = 4 (D + 2) 2^-24 (|x_n|^2 + max_m |p_m|^2): how far the true distance of a returned neighbour may lie from the oracle's distance
    of the same rank.  An fp32 dot product of D terms plus h is off by at most (D + 2) 2^-24 (|x||p| + |p|^2 / 2) <= (D + 2) 2^-24
    (|x|^2 + |p|^2) per score; two scores decide an order and d = |x|^2 - 2 s doubles their gap: the factor 4."""
    D = X.shape[1]
    x2 = (X.astype(np.float64) ** 2).sum(1)
    p2 = (P.astype(np.float64) ** 2).sum(1).max()
    return 4.0 * (D + 2) * 2.0 ** -24 * (x2 + p2)


def blend_bound(X, P):
    """|y - y64| <= 8 (D + 4) 2^-24 max(|X|inf, |P|inf): a sum of D squares carries a relative error of (D + 1) 2^-24, the reciprocal, the
    square and the two normalisations a few more units, so every weight is off by at most ~2 (D + 4) 2^-24 relatively (the square doubles the
    distance's error); z is a convex combination of rows bounded by |P|inf, the chain over k <= 8 rows and the final blend add less than
    the remaining factor."""
    D = X.shape[1]
    return 8.0 * (D + 4) * 2.0 ** -24 * max(np.abs(X).max(), np.abs(P).max())
