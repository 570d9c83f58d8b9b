"""Units retrieval: the "units index" of the Diffusion-SVC / RVC tool chains (there an approximate faiss index on the host), exact and on
the HIP device (include/lds.h lds_knn_*, csrc/knn.hip).  Before the units go into Unit2Mel every frame is pulled towards its k nearest frames
in a pool of the target speaker's units: y = (1 - ratio) x + ratio sum_j w_j p_j, w_j ~ 1 / d_j^2 over the squared distances d_j.

`units_index.pt` is a torch-saved dict {"pool": float32 ndarray [M, D], "n_features_in_": D, "source_rows": int, "reduced": bool}
(tools/train_units_index.py writes it; `source_rows` / `reduced` record whether the pool is the speaker's frames or their k-means centres)."""
import numpy as np
import torch

MAX_K = 8
MAX_ROWS = 16777216


class UnitsIndex:
    def __init__(self, pool, source_rows=None, reduced=False):
        """pool: numpy or tensor [M, D] (D a multiple of 8 in 8 .. 4096, M <= 16,777,216); a device tensor is used where it is, anything
        else is uploaded on first use on a device"""
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
            self._on[key] = (p, native.knn_prepare(p))
        return self._on[key]

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

    def search(self, x, k=8):
        """x [.., D] on the device -> (idx int64 [.., k], score [.., k]): the k nearest pool rows of every frame, nearest first, the lower
        index among exactly equal scores; score = x.p - |p|^2 / 2 (|x|^2 - 2 score is the squared distance)"""
        from lds import native
        k = self._check(x, k, (1, 2, 3))
        x = self._on_device(x)
        pool, h = self._device(x.device)
        idx, score = native.knn_search(x.reshape(-1, x.shape[-1]), pool, h, k)
        return idx.to(torch.int64).reshape(*x.shape[:-1], k), score.reshape(*x.shape[:-1], k)

    def retrieve(self, x, k=8, ratio=0.5, lengths=None, return_neighbours=False):
        """x [N, D] or [B, T, D] on the device -> y of the same shape; lengths ([B] ints, 0 .. T; needs [B, T, D], B <= 64): rows at and
        beyond a clip's length come back as zeros.  return_neighbours: (y, idx int64 [.., k], dist [.., k]) with the squared distances
        (floored at 1e-12) that the weights were formed from; idx = -1 beyond a clip's length"""
        from lds import native
        k = self._check(x, k, (2, 3))
        if isinstance(ratio, bool) or not isinstance(ratio, (int, float)) or not 0.0 <= ratio <= 1.0:      # (NaN fails the comparison)
            raise ValueError(f"UnitsIndex: ratio must be a number in 0 .. 1 (got {ratio!r})")
        if lengths is not None:
            if x.dim() != 3:
                raise ValueError("UnitsIndex: lengths= needs x [B, T, D]")
            lengths = native._host_lengths(lengths, x.shape[0], 0, x.shape[1], max_B=64, what="retrieval")
        x = self._on_device(x)
        pool, h = self._device(x.device)
        if lengths is None:
            y, idx, dist = native.knn_retrieve(x.reshape(-1, x.shape[-1]), pool, h, k, ratio)
            y, idx, dist = y.reshape(x.shape), idx.reshape(*x.shape[:-1], k), dist.reshape(*x.shape[:-1], k)
        else:
            y, idx, dist = native.knn_retrieve(x, pool, h, k, ratio, lengths=lengths)
        return (y, idx.to(torch.int64), dist) if return_neighbours else y

    def state(self):
        pool = self.pool.cpu().numpy() if isinstance(self.pool, torch.Tensor) else self.pool
        return {"pool": np.ascontiguousarray(pool, dtype=np.float32), "n_features_in_": self.n_features_in_, "source_rows": self.source_rows,
                "reduced": self.reduced}

    def save(self, path):
        torch.save(self.state(), path)

    @classmethod
    def load(cls, path):
        ck = torch.load(path, map_location="cpu", weights_only=False)      # a numpy array inside: not a weights-only file
        ix = cls(ck["pool"], source_rows=ck.get("source_rows"), reduced=ck.get("reduced", False))
        if int(ck.get("n_features_in_", ix.n_features_in_)) != ix.n_features_in_:
            raise ValueError(f"{path}: n_features_in_ {ck['n_features_in_']} against a pool of width {ix.n_features_in_}")
        return ix
