"""KMeansGPU with the reference's name, arguments and control flow (reference cluster/kmeans.py:51-206), on liblds' k-means kernels
(include/lds.h lds_kmeans_*): k-means++ seeding, the assignment on the fp32 MFMA and the Lloyd step all run on the HIP device; torch
owns the memory and draws the random numbers.

Deviations from the reference, all deliberate:
  * the free-memory figure behind `minibatch` comes from torch.cuda.mem_get_info (the reference asks pynvml, which needs an NVIDIA
    device); keyword-only `minibatch=` overrides it and `init=` passes starting centroids (no seeding, no seeding draws);
  * every random draw comes from torch's CPU generator (the reference draws _kpp's subsample on the data's device), in the
    reference's order: the seeding subset, _kpp's own subsample, its first index, its K - 1 uniforms, then the fit's subsets;
  * a seeding draw that rounding leaves above the last cumulative probability picks the last point (the reference raises IndexError);
  * labels are int64 (the reference's int16 wraps above 32,767 codes);
  * the reference's second mode is a class of its own, KMeansCosineGPU: KMeansGPU(mode="cosine") keeps the refusal it always gave (and the
    constructor its signature), the subclass runs that mode.

KMeansCosineGPU (the reference's mode="cosine", kmeans.py:96-105 cos_sim) assigns by (x . c) / max(|c|, 1e-12) -- the per-centre constant
sits where |c|^2 / 2 sits in Euclidean mode, no normalised copy of the data or the centres is made -- and reports the cosine similarity; the
Lloyd step and the k-means++ seeding are the Euclidean mode's, as in the reference."""
import numpy as np
import torch

from lds import native


def _kpp(data, k, sample_size=-1):
    """k-means++ starting centroids of `data` [n, dim] on the device (reference kmeans.py:10-50)"""
    batch_size = data.shape[0]
    if batch_size > sample_size:
        data = data[torch.randint(0, batch_size, [sample_size]).to(data.device)].contiguous()
    first = int(torch.randint(data.shape[0], [1]))
    r = torch.distributions.uniform.Uniform(0, 1)
    u = torch.cat([r.sample([1]) for _ in range(k - 1)]) if k > 1 else torch.zeros(0)
    return native.kmeans_seed(data, k, first, u.to(torch.float32).to(data.device))[0]


class KMeansGPU:
    _metric = "l2"      # what the assignment goes by (lds.native's name); KMeansCosineGPU: "cosine"

    def __init__(self, n_clusters, max_iter=200, tol=1e-4, verbose=0, mode="euclidean", device=torch.device("cuda:0"), *, minibatch=None, init=None):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("KMeansGPU needs a HIP device (no CPU fallback for the hot path)")
        if mode != "euclidean":
            raise NotImplementedError(f"KMeansGPU: mode {mode!r} is not built (only 'euclidean'); the reference's mode 'cosine' is KMeansCosineGPU")
        self.n_clusters = n_clusters
        self.max_iter = max_iter
        self.tol = tol
        self.verbose = verbose
        self.mode = mode
        self.init = init
        if minibatch is None:
            free = torch.cuda.mem_get_info(self.device)[0]
            minibatch = int(33e6 / self.n_clusters * free / 1024 / 1024 / 1024)
        self.minibatch = int(minibatch)
        self.centroids = None
        self.n_iter_ = 0
        self.errors_ = []

    @staticmethod
    def euc_sim(a, b):
        raise NotImplementedError("the n x k similarity matrix is never formed: use max_sim")

    @staticmethod
    def cos_sim(a, b):
        raise NotImplementedError("the n x k similarity matrix is never formed: use max_sim")

    def max_sim(self, a, b):
        """(max_k euc_sim(a, b), its index): 2 a.b - |a|^2 - |b|^2 of the nearest row of b, lowest index among ties; in cosine mode
        (max_k cos_sim(a, b), its index): the cosine similarity of the best row of b, any number of rows of a"""
        a = a.to(self.device, torch.float32).contiguous()
        b = b.to(self.device, torch.float32).contiguous()
        if self._metric == "cosine":
            idx, best = native.kmeans_assign(a, b, native.kmeans_prepare(b, "cosine"), return_best=True, metric="cosine")
            return best, idx
        idx, best = native.kmeans_assign(a, b, native.kmeans_prepare(b), return_best=True)
        # |a_n|^2 / 2 by the same kernel, 65,536 rows (its codebook limit) at a time: `a` may hold millions of rows
        ha = torch.cat([native.kmeans_prepare(a[r:r + 65536]) for r in range(0, a.shape[0], 65536)])
        return native.axpby(best, ha, 2.0, -2.0), idx

    def fit_predict(self, X):
        assert isinstance(X, torch.Tensor), "input must be torch.Tensor"
        assert X.dtype in [torch.half, torch.float, torch.double], "input must be floating point"
        assert X.ndim == 2, "input must be a 2d tensor with shape: [n_samples, n_features] "
        K, dev = self.n_clusters, self.device
        to_dev = lambda t: t.to(dev, torch.float32).contiguous()
        offset = np.power(1.5, np.log(K / 1000)) / np.log(2)
        with torch.no_grad():
            batch_size = X.shape[0]
            if self.init is None:
                if self.minibatch * 10 // offset < batch_size:
                    x = to_dev(X[torch.randint(0, batch_size, [int(self.minibatch * 10 / offset)]).to(X.device)])
                else:
                    x = to_dev(X)
                self.centroids = _kpp(x, K, min(int(self.minibatch / 12 / offset), batch_size))
                del x
            else:
                self.centroids = to_dev(torch.as_tensor(self.init)).clone()
                if tuple(self.centroids.shape) != (K, X.shape[1]):
                    raise ValueError(f"init must be [{K}, {X.shape[1]}]")
            h = native.kmeans_prepare(self.centroids, self._metric)
            num_points = torch.ones(K, device=dev, dtype=torch.float32)
            closest = None
            if self.minibatch >= batch_size // 2 and self.minibatch < batch_size:
                X = to_dev(X[torch.randint(0, batch_size, [self.minibatch]).to(X.device)])
            elif self.minibatch >= batch_size:
                X = to_dev(X)
            self.errors_ = []
            for i in range(self.max_iter):
                if self.minibatch < batch_size // 2:
                    x = to_dev(X[torch.randint(0, batch_size, [self.minibatch]).to(X.device)])
                else:
                    x = X
                closest = native.kmeans_assign(x, self.centroids, h, metric=self._metric)
                error = native.kmeans_update(x, closest, self.centroids, h, num_points, metric=self._metric).item()      # the one 4-byte read per iteration
                self.errors_.append(error)
                if self.verbose >= 2:
                    print("iter:", i, "error:", error)
                if error <= self.tol:
                    break
            self.n_iter_ = len(self.errors_)
            if self.verbose >= 1:
                print(f"used {self.n_iter_} iterations to cluster {batch_size} items into {K} clusters")
        return closest


class KMeansCosineGPU(KMeansGPU):
    """The reference's KMeansGPU(mode="cosine"): the same arguments without `mode`, the same fit loop, the assignment by cosine similarity
    (`max_sim` returns that similarity)."""
    _metric = "cosine"

    def __init__(self, n_clusters, max_iter=200, tol=1e-4, verbose=0, device=torch.device("cuda:0"), *, minibatch=None, init=None):
        super().__init__(n_clusters, max_iter=max_iter, tol=tol, verbose=verbose, device=device, minibatch=minibatch, init=init)
        self.mode = "cosine"
