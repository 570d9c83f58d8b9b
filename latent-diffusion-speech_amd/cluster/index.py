"""Units retrieval: the "units index" of the Diffusion-SVC / RVC tool chains (there an approximate faiss index on the host), exact and on
the HIP device (include/lds.h lds_knn_*, csrc/knn.hip).  Before the units go into Unit2Mel every frame is pulled towards its k nearest frames
in a pool of the target speaker's units: y = (1 - ratio) x + ratio sum_j w_j p_j, w_j ~ 1 / d_j^2 over the squared distances d_j.

`units_index.pt` is a torch-saved dict {"pool": float32 ndarray [M, D], "n_features_in_": D, "source_rows": int, "reduced": bool}
(tools/train_units_index.py writes it; `source_rows` / `reduced` record whether the pool is the speaker's frames or their k-means centres).

An IVF coarse index (`build_ivf`; include/lds.h lds_ivf_*, faiss IndexIVFFlat's role in those tool chains) groups the pool's rows by their
nearest of `nlist` coarse centres; `search` / `retrieve` with `nprobe=` then score a frame against the rows of its nprobe best centres only.
The file then carries one more key, "ivf": {"centres": float32 [nlist, D], "offsets": int64 [nlist + 1], "order": int32 [M]}.

metric="cosine" is kNN-VC's matching: neighbours by cosine similarity (score (x . p) / max(|p|, 1e-12), one constant per pool row -- no
normalised copy of the pool), distances 1 - cos; `retrieve(weights="uniform")` is its plain mean of the matched ORIGINAL rows.  The file
carries "metric": "cosine" (an l2 index writes no such key, and a file without it is l2); an IVF belongs to the metric it was built under."""
import numpy as np
import torch

MAX_K = 8
MAX_ROWS = 16777216
MAX_NPROBE = 8
MAX_NLIST = 65536
METRICS = ("l2", "cosine")
WEIGHTS = ("inverse_square", "uniform")
BLOCK = 128      # the list-ordered copy pads every list to whole blocks of this many rows


def _assign_lists(pool, centres, device, metric="l2"):
    """labels int64 numpy [M]: every pool row's best centre by lds_kmeans_assign (score p.c - |c|^2 / 2, or the cosine score (p.c) / |c|; the
    lower centre among equal scores)"""
    from lds import native
    if torch.device(device).type != "cuda":
        raise RuntimeError("UnitsIndex.build_ivf needs a HIP device (no CPU fallback for the assignment)")
    p = (pool if isinstance(pool, torch.Tensor) else torch.from_numpy(pool)).to(device).contiguous()
    c = torch.as_tensor(centres, dtype=torch.float32).to(device).contiguous()
    return native.kmeans_assign(p, c, native.kmeans_prepare(c, metric), metric=metric).cpu().numpy()


def _fit_centres(pool, nlist, max_iter, seed, device, metric="l2"):
    """nlist k-means centres of the pool by the project's KMeansGPU (seeded), in the index's metric"""
    from .kmeans import KMeansCosineGPU, KMeansGPU
    torch.manual_seed(seed)
    km = (KMeansCosineGPU if metric == "cosine" else KMeansGPU)(n_clusters=nlist, max_iter=max_iter, device=torch.device(device))
    km.fit_predict(pool if isinstance(pool, torch.Tensor) else torch.from_numpy(pool))
    return km.centroids.cpu().numpy()


class UnitsIndex:
    def __init__(self, pool, source_rows=None, reduced=False, metric="l2"):
        """pool: numpy or tensor [M, D] (D a multiple of 8 in 8 .. 4096, M <= 16,777,216); a device tensor is used where it is, anything
        else is uploaded on first use on a device.  metric: "l2" or "cosine" -- what search, retrieve, probe_lists and build_ivf go by"""
        if not isinstance(metric, str) or metric not in METRICS:
            raise ValueError(f"UnitsIndex: metric must be one of {list(METRICS)} (got {metric!r})")
        self.metric = metric
        if isinstance(pool, torch.Tensor):
            pool = pool.detach().to(torch.float32).contiguous()
        else:
            pool = np.ascontiguousarray(pool, dtype=np.float32)
        if pool.ndim != 2 or pool.shape[0] < 1 or pool.shape[0] > MAX_ROWS:
            raise ValueError(f"UnitsIndex: the pool must be [M, D] with 1 <= M <= {MAX_ROWS} (got {list(pool.shape)})")
        if pool.shape[1] % 8 or not 8 <= pool.shape[1] <= 4096:
            raise ValueError(f"UnitsIndex: the width {pool.shape[1]} must be a multiple of 8 in 8 .. 4096")
        self.pool = pool
        self.n_features_in_ = int(pool.shape[1])
        self.source_rows = int(pool.shape[0] if source_rows is None else source_rows)
        self.reduced = bool(reduced)
        self._on = {}      # device string -> (pool on the device, h)
        self.ivf = None    # build_ivf / load: {"centres" float32 [nlist, D], "offsets" int64 [nlist + 1], "order" int32 [M]} (numpy)
        self._ivf_on = {}  # device string -> (centres, hc, offsets, order, list-ordered copy, its h) on the device

    def __len__(self):
        return int(self.pool.shape[0])

    def _device(self, device):
        """(pool [M, D], h [M]) on `device`: uploaded and prepared once per device"""
        from lds import native
        key = str(device)
        if key not in self._on:
            if torch.device(device).type != "cuda":
                raise RuntimeError("UnitsIndex needs tensors on a HIP device (no CPU fallback for the hot path)")
            p = self.pool if isinstance(self.pool, torch.Tensor) else torch.from_numpy(self.pool)
            p = p.to(device).contiguous()
            self._on[key] = (p, native.knn_prepare(p, self.metric))
        return self._on[key]

    @property
    def nlist(self):
        return 0 if self.ivf is None else int(self.ivf["centres"].shape[0])

    def build_ivf(self, nlist, *, centres=None, max_iter=25, seed=0, device="cuda"):
        """Group the pool's rows into lists by their nearest coarse centre.  Without `centres` nlist centres are fitted to the pool with
        KMeansGPU (max_iter, seed); with centres [L, D] (L = nlist) the rows are only assigned.  Lists that receive no row are dropped with
        their centre (self.nlist is what is left); inside a list the rows keep ascending original index.  Returns self."""
        if isinstance(nlist, bool) or not isinstance(nlist, (int, np.integer)) or not 1 <= nlist <= min(MAX_NLIST, len(self)):
            raise ValueError(f"UnitsIndex: nlist must be an integer in 1 .. min({MAX_NLIST}, the pool's {len(self)} rows) (got {nlist!r})")
        how = {} if self.metric == "l2" else {"metric": self.metric}      # (the l2 calls are the ones that were always made)
        if centres is None:
            centres = _fit_centres(self.pool, int(nlist), max_iter, seed, device, **how)
        else:
            centres = centres.detach().cpu().numpy() if isinstance(centres, torch.Tensor) else np.asarray(centres)
        centres = np.ascontiguousarray(centres, dtype=np.float32)
        if centres.shape != (nlist, self.n_features_in_):
            raise ValueError(f"UnitsIndex: centres {list(centres.shape)} must be [{nlist}, {self.n_features_in_}]")
        labels = np.asarray(_assign_lists(self.pool, centres, device, **how)).reshape(-1)
        counts = np.bincount(labels, minlength=nlist)
        keep = np.flatnonzero(counts)
        self._set_ivf({"centres": centres[keep], "offsets": np.concatenate([[0], np.cumsum(counts[keep])]),
                       "order": np.argsort(labels, kind="stable")})
        return self

    def _set_ivf(self, ivf):
        centres = np.ascontiguousarray(ivf["centres"], dtype=np.float32)
        offsets = np.ascontiguousarray(ivf["offsets"], dtype=np.int64)
        order = np.ascontiguousarray(ivf["order"], dtype=np.int32)
        L = centres.shape[0]
        if (centres.ndim != 2 or centres.shape[1] != self.n_features_in_ or not 1 <= L <= MAX_NLIST or offsets.shape != (L + 1,)
                or order.shape != (len(self),) or offsets[0] != 0 or offsets[-1] != len(self) or (np.diff(offsets) < 1).any()
                or not np.array_equal(np.sort(order), np.arange(len(self)))):
            raise ValueError("UnitsIndex: the IVF tables do not describe this pool (centres [nlist, D], offsets [nlist + 1] from 0 to M with no "
                             "empty list, order a permutation of the M rows)")
        self.ivf = {"centres": centres, "offsets": offsets, "order": order}
        self._ivf_on = {}

    def _device_ivf(self, device):
        """the IVF on `device`: (centres, hc, offsets, order, the pool in list order with every list padded to whole blocks, its h)"""
        from lds import native
        key = str(device)
        if key not in self._ivf_on:
            pool, h = self._device(device)
            offsets, order = self.ivf["offsets"], self.ivf["order"]
            lens = np.diff(offsets)
            blocks = (lens + BLOCK - 1) // BLOCK
            first = np.concatenate([[0], np.cumsum(blocks)[:-1]]) * BLOCK      # every list's first row in the copy
            at = torch.from_numpy(np.repeat(first - offsets[:-1], lens) + np.arange(len(self))).to(device)
            od = torch.from_numpy(order).to(device)
            copy = torch.zeros(int(blocks.sum()) * BLOCK, self.n_features_in_, dtype=torch.float32, device=device)
            hl = torch.zeros(copy.shape[0], dtype=torch.float32, device=device)
            copy[at] = pool[od.long()]
            hl[at] = h[od.long()]
            centres = torch.from_numpy(self.ivf["centres"]).to(device)
            self._ivf_on[key] = (centres, native.knn_prepare(centres, self.metric), torch.from_numpy(offsets).to(device), od, copy, hl)
        return self._ivf_on[key]

    def _check_nprobe(self, nprobe):
        if self.ivf is None:
            raise ValueError("UnitsIndex: nprobe= needs an IVF (build_ivf, or an index file written with one)")
        if isinstance(nprobe, bool) or not isinstance(nprobe, (int, np.integer)) or not 1 <= nprobe <= min(MAX_NPROBE, self.nlist):
            raise ValueError(f"UnitsIndex: nprobe must be an integer in 1 .. min({MAX_NPROBE}, the index's {self.nlist} lists) (got {nprobe!r})")
        return int(nprobe)

    def probe_lists(self, x, nprobe):
        """x [.., D] on the device -> int64 [.., nprobe]: the lists an `nprobe` search of x scores, best centre first"""
        from lds import native
        nprobe = self._check_nprobe(nprobe)
        if not isinstance(x, torch.Tensor):
            raise RuntimeError("UnitsIndex needs a tensor on a HIP device (numpy input: no CPU fallback for the hot path)")
        if x.dim() not in (1, 2, 3) or x.shape[-1] != self.n_features_in_ or x.numel() == 0:
            raise ValueError(f"UnitsIndex: x {list(x.shape)} against a pool of width {self.n_features_in_}")
        x = self._on_device(x)
        centres, hc = self._device_ivf(x.device)[:2]
        return native.knn_search(x.reshape(-1, x.shape[-1]), centres, hc, nprobe, metric=self.metric)[0].to(torch.int64).reshape(*x.shape[:-1], nprobe)

    def _check(self, x, k, dims):
        """the argument checks of search / retrieve, the ValueErrors first: they do not depend on where x lives"""
        if not isinstance(x, torch.Tensor):
            raise RuntimeError("UnitsIndex needs a tensor on a HIP device (numpy input: no CPU fallback for the hot path)")
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= min(MAX_K, len(self)):
            raise ValueError(f"UnitsIndex: k must be an integer in 1 .. min({MAX_K}, the pool's {len(self)} rows) (got {k!r})")
        if x.dim() not in dims or x.shape[-1] != self.n_features_in_ or x.numel() == 0:
            raise ValueError(f"UnitsIndex: x {list(x.shape)} against a pool of width {self.n_features_in_}")
        return int(k)

    @staticmethod
    def _on_device(x):
        if not x.is_cuda:
            raise RuntimeError("UnitsIndex needs a tensor on a HIP device (no CPU fallback for the hot path)")
        return x.to(torch.float32).contiguous()

    def search(self, x, k=8, nprobe=None):
        """x [.., D] on the device -> (idx int64 [.., k], score [.., k]): the k nearest pool rows of every frame, nearest first, the lower
        index among exactly equal scores; score = x.p - |p|^2 / 2 (|x|^2 - 2 score is the squared distance), or the cosine similarity of a
        cosine index.  nprobe (needs build_ivf): only
        the rows of the frame's nprobe best lists are scored; -1 / -inf where they hold fewer than k rows"""
        from lds import native
        k = self._check(x, k, (1, 2, 3))
        if nprobe is not None:
            nprobe = self._check_nprobe(nprobe)
        x = self._on_device(x)
        pool, h = self._device(x.device)
        if nprobe is None:
            idx, score = native.knn_search(x.reshape(-1, x.shape[-1]), pool, h, k, metric=self.metric)
        else:
            idx, score = native.ivf_search(x.reshape(-1, x.shape[-1]), pool, h, k, self._device_ivf(x.device), nprobe, metric=self.metric)
        return idx.to(torch.int64).reshape(*x.shape[:-1], k), score.reshape(*x.shape[:-1], k)

    def retrieve(self, x, k=8, ratio=0.5, lengths=None, return_neighbours=False, nprobe=None, weights="inverse_square"):
        """x [N, D] or [B, T, D] on the device -> y of the same shape; lengths ([B] ints, 0 .. T; needs [B, T, D], B <= 64): rows at and
        beyond a clip's length come back as zeros.  return_neighbours: (y, idx int64 [.., k], dist [.., k]) with the squared distances
        (floored at 1e-12) that the weights were formed from; idx = -1 beyond a clip's length.  nprobe (needs build_ivf): the neighbours come
        from the frame's nprobe best lists; where those hold fewer than k rows idx = -1 and the blend is over the rows found.
        weights: "inverse_square" (w_j ~ 1 / d_j^2) or "uniform" (the plain mean of the rows found: kNN-VC's).  A cosine index reports
        dist = 1 - cos; the blend is over the pool's original rows whatever the metric"""
        from lds import native
        if not isinstance(weights, str) or weights not in WEIGHTS:
            raise ValueError(f"UnitsIndex: weights must be one of {list(WEIGHTS)} (got {weights!r})")
        k = self._check(x, k, (2, 3))
        if nprobe is not None:
            nprobe = self._check_nprobe(nprobe)
        if isinstance(ratio, bool) or not isinstance(ratio, (int, float)) or not 0.0 <= ratio <= 1.0:      # (NaN fails the comparison)
            raise ValueError(f"UnitsIndex: ratio must be a number in 0 .. 1 (got {ratio!r})")
        if lengths is not None:
            if x.dim() != 3:
                raise ValueError("UnitsIndex: lengths= needs x [B, T, D]")
            lengths = native._host_lengths(lengths, x.shape[0], 0, x.shape[1], max_B=64, what="retrieval")
        x = self._on_device(x)
        pool, h = self._device(x.device)
        if nprobe is None:
            run = lambda x, **kw: native.knn_retrieve(x, pool, h, k, ratio, metric=self.metric, weights=weights, **kw)      # noqa: E731
        else:
            ivf = self._device_ivf(x.device)
            run = lambda x, **kw: native.ivf_retrieve(x, pool, h, k, ratio, ivf, nprobe, metric=self.metric, weights=weights, **kw)      # noqa: E731
        if lengths is None:
            y, idx, dist = run(x.reshape(-1, x.shape[-1]))
            y, idx, dist = y.reshape(x.shape), idx.reshape(*x.shape[:-1], k), dist.reshape(*x.shape[:-1], k)
        else:
            y, idx, dist = run(x, lengths=lengths)
        return (y, idx.to(torch.int64), dist) if return_neighbours else y

    def state(self):
        pool = self.pool.cpu().numpy() if isinstance(self.pool, torch.Tensor) else self.pool
        st = {"pool": np.ascontiguousarray(pool, dtype=np.float32), "n_features_in_": self.n_features_in_, "source_rows": self.source_rows,
              "reduced": self.reduced}
        if self.metric != "l2":      # (an l2 index writes the file it always wrote; a file without the key is l2)
            st["metric"] = self.metric
        if self.ivf is not None:
            st["ivf"] = dict(self.ivf)
        return st

    def save(self, path):
        torch.save(self.state(), path)

    @classmethod
    def load(cls, path):
        ck = torch.load(path, map_location="cpu", weights_only=False)      # a numpy array inside: not a weights-only file
        ix = cls(ck["pool"], source_rows=ck.get("source_rows"), reduced=ck.get("reduced", False), metric=ck.get("metric", "l2"))
        if int(ck.get("n_features_in_", ix.n_features_in_)) != ix.n_features_in_:
            raise ValueError(f"{path}: n_features_in_ {ck['n_features_in_']} against a pool of width {ix.n_features_in_}")
        if ck.get("ivf") is not None:
            ix._set_ivf(ck["ivf"])
        return ix
