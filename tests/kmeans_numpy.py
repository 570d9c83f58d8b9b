"""Float64 restatement of the k-means tokenizer for the tests (not a product path; the product's is csrc/kmeans.hip):
nearest-centre assignment with its error bound, the reference's Lloyd step (cluster/kmeans.py:184-202), its fit loop, and k-means++
seeding with a running minimum (kmeans.py:42-49).  Inputs are regenerated from seeds, never stored."""
import numpy as np

U24 = 2.0 ** -24


def make_blobs(seed, K, D, N, spread=0.5):
    """centres N(0,1) [K, D], points = a centre + spread * N(0,1) [N, D] (float32), the planted labels [N]; spread None: pure N(0,1) points"""
    rng = np.random.default_rng(seed)
    C = rng.standard_normal((K, D)).astype(np.float32)
    if spread is None:
        return C, rng.standard_normal((N, D)).astype(np.float32), None
    lab = rng.integers(0, K, N)
    X = (C[lab] + np.float32(spread) * rng.standard_normal((N, D)).astype(np.float32)).astype(np.float32)
    return C, X, lab


def sqdist64(X, C, rows=512):
    """yields (r0, d [rows, K]) of the squared distances in float64, as differences (no cancellation)"""
    X64, C64 = np.asarray(X, np.float64), np.asarray(C, np.float64)
    cn = (C64 * C64).sum(1)
    for r0 in range(0, X64.shape[0], rows):
        x = X64[r0:r0 + rows]
        yield r0, np.maximum((x * x).sum(1)[:, None] - 2.0 * (x @ C64.T) + cn[None, :], 0.0)


def assign64(X, C):
    """(labels = float64 arg-min of the squared distance, lowest index among ties; gap = runner-up distance - best distance)"""
    N = len(X)
    lab, gap = np.empty(N, np.int64), np.empty(N, np.float64)
    for r0, d in sqdist64(X, C):
        l = d.argmin(1)
        lab[r0:r0 + len(l)] = l
        if d.shape[1] > 1:
            part = np.partition(d, 1, axis=1)
            gap[r0:r0 + len(l)] = part[:, 1] - part[:, 0]
        else:
            gap[r0:r0 + len(l)] = np.inf
    return lab, gap


def eps_bound(X, C):
    """eps(n) = 4 (D + 2) 2^-24 |x_n| max_k |c_k| + 4 2^-24 max_k |c_k|^2: the a-priori bound on how much farther (squared distance) than the
    true nearest centre an fp32 arg-max of x.c - |c|^2/2 may land (derivation: tests/test_gpu_kmeans.py test_assign_criterion)"""
    X64, C64 = np.asarray(X, np.float64), np.asarray(C, np.float64)
    D = X64.shape[1]
    cmax = np.sqrt((C64 * C64).sum(1).max())
    return 4.0 * (D + 2) * U24 * np.sqrt((X64 * X64).sum(1)) * cmax + 4.0 * U24 * cmax * cmax


def excess64(X, C, labels):
    """d(x_n, c_label) - min_k d(x_n, c_k) in float64, per row"""
    out = np.empty(len(X), np.float64)
    labels = np.asarray(labels)
    for r0, d in sqdist64(X, C):
        l = labels[r0:r0 + len(d)]
        out[r0:r0 + len(d)] = d[np.arange(len(d)), l] - d.min(1)
    return out


def lloyd_step64(X, labels, C, num_points):
    """one iteration of kmeans.py:185-198 given the labels -> (C', num_points', error, c_grad), float64"""
    X64, C64 = np.asarray(X, np.float64), np.asarray(C, np.float64)
    K = C64.shape[0]
    counts = np.bincount(labels, minlength=K).astype(np.float64)
    sums = np.zeros_like(C64)
    np.add.at(sums, labels, X64)
    with np.errstate(invalid="ignore", divide="ignore"):
        c_grad = sums / counts[:, None]
    c_grad[counts == 0] = 0.0
    error = ((c_grad - C64) ** 2).sum()
    lr = 1.0 / np.asarray(num_points, np.float64)[:, None] * 0.9 + 0.1
    return C64 * (1 - lr) + c_grad * lr, np.asarray(num_points, np.float64) + counts, error, c_grad


def fit64(X, C0, max_iter, tol, batches=None):
    """the loop of kmeans.py:177-202 from a given start; batches: None (full batch) or a callable i -> row indices of iteration i's subset.
    -> dict(labels per iteration, errors, centroids, n_iter)"""
    C, npnt = np.asarray(C0, np.float64), np.ones(len(C0))
    labels, errors = [], []
    for i in range(max_iter):
        x = X if batches is None else X[batches(i)]
        lab = assign64(x, C)[0]
        C, npnt, err, _ = lloyd_step64(x, lab, C, npnt)
        labels.append(lab)
        errors.append(err)
        if err <= tol:
            break
    return {"labels": labels, "errors": np.array(errors), "centroids": C, "n_iter": len(errors), "num_points": npnt}


def kpp64(X, K, first, uniforms):
    """k-means++ picks with a running minimum: weight = Euclidean distance (not squared) to the nearest picked centre, pick = first j with
    cumsum(w / sum w)[j] >= u (searchsorted left), clamped to N - 1.  -> (picks [K], clearance [K-1] = distance of every draw to the nearest
    CDF boundary)"""
    X64 = np.asarray(X, np.float64)
    picks, clear = [int(first)], []
    mind = None
    for i in range(1, K):
        d = np.sqrt(((X64 - X64[picks[-1]]) ** 2).sum(1))
        mind = d if mind is None else np.minimum(mind, d)
        cum = np.cumsum(mind / mind.sum())
        u = float(uniforms[i - 1])
        j = min(int(np.searchsorted(cum, u, side="left")), len(X64) - 1)
        picks.append(j)
        clear.append(np.abs(cum - u).min())
    return np.array(picks), np.array(clear)


def kpp_interval(X, picks_so_far):
    """float64 CDF of the next pick given the picks so far -> cum [N] (cum[j-1] < u <= cum[j] picks j)"""
    X64 = np.asarray(X, np.float64)
    mind = np.full(len(X64), np.inf)
    for p in picks_so_far:
        mind = np.minimum(mind, np.sqrt(((X64 - X64[p]) ** 2).sum(1)))
    return np.cumsum(mind / mind.sum())
