"""Build a units index: the pool of a target speaker's unit frames that cluster.index.UnitsIndex searches (infer_svc.py / infer_tts.py --index).

    python tools/train_units_index.py UNITS_DIR -o units_index.pt [--max_rows 200000] [--reduce_to 10000] [--max_files 30000] [--seed 0]
                                      [--max_iter 100] [--tol 1e-2] [--synthetic M] [--nlist 0] [--nlist_iter 25]

UNITS_DIR holds .npy unit files [T, dim] (tools/extract_units.py writes them), searched recursively and read as tools/train_codebook.py
reads them: up to --max_files of them, shuffled with --seed, concatenated.  Up to --max_rows frames the pool is the frames themselves
(the search is exact at any size; 16,777,216 rows at the most).  Above --max_rows the pool is reduced to --reduce_to k-means centres of
the frames by cluster.train_cluster (the codebook fit, on the HIP device) -- what the faiss-based tool chains do with a large speaker.
--synthetic M: M seeded Gaussian rows of the files' width instead of the frames (a stand-in pool for smoke runs).
--nlist N (default 0: none): an IVF coarse index over the pool as well -- N k-means centres of the pool (cluster.train_cluster, --nlist_iter
iterations) and every row's list (UnitsIndex.build_ivf), so that --index_nprobe searches a few lists instead of the pool and a large speaker
keeps its frames: raise --max_rows with it.
The file is a torch-saved dict {"pool": float32 [M, D], "n_features_in_": D, "source_rows": the frames read, "reduced": bool}, with --nlist
also "ivf": {"centres", "offsets", "order"}.
"""
import argparse
import glob
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "latent-diffusion-speech_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import cluster  # noqa: E402
from cluster.index import UnitsIndex  # noqa: E402


def _mode(metric):
    """train_cluster's extra arguments for an index metric: none for l2 (the call that was always made), mode="cosine" for cosine"""
    return {} if metric == "l2" else {"mode": "cosine"}


def build_pool(feats, max_rows, reduce_to, seed=0, max_iter=100, tol=1e-2, metric="l2"):
    """feats [n, dim] -> (pool, reduced): the frames themselves up to max_rows, else reduce_to k-means centres of them (cosine k-means
    for a cosine index)"""
    if feats.shape[0] <= max_rows:
        return np.ascontiguousarray(feats, dtype=np.float32), False
    if not 1 <= reduce_to <= max_rows:
        raise ValueError(f"--reduce_to {reduce_to} outside 1 .. --max_rows {max_rows}")
    torch.manual_seed(seed)
    ck = cluster.train_cluster(feats, reduce_to, max_iter=max_iter, tol=tol, **_mode(metric))
    return np.ascontiguousarray(ck["cluster_centers_"], dtype=np.float32), True


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("units_dir")
    ap.add_argument("-o", "--out", default="units_index.pt")
    ap.add_argument("--max_rows", type=int, default=200000)
    ap.add_argument("--reduce_to", type=int, default=10000)
    ap.add_argument("--max_files", type=int, default=30000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max_iter", type=int, default=100)
    ap.add_argument("--tol", type=float, default=1e-2)
    ap.add_argument("--synthetic", type=int, default=0, metavar="M")
    ap.add_argument("--nlist", type=int, default=0, help="lists of an IVF coarse index over the pool (0: none)")
    ap.add_argument("--nlist_iter", type=int, default=25)
    ap.add_argument("--metric", default="l2", choices=("l2", "cosine"), help="cosine: kNN-VC's matching (the reduction and the IVF then use cosine k-means); "
                    "the file records it and infer_svc.py / infer_tts.py follow it")
    a = ap.parse_args(argv)
    paths = sorted(glob.glob(os.path.join(a.units_dir, "**", "*.npy"), recursive=True))
    if not paths:
        raise SystemExit(f"no .npy unit files under {a.units_dir}")
    random.Random(a.seed).shuffle(paths)
    feats = np.concatenate([np.load(p).astype(np.float32) for p in paths[: a.max_files]], axis=0)
    if a.synthetic:
        pool, reduced = np.random.default_rng(a.seed).standard_normal((a.synthetic, feats.shape[1])).astype(np.float32), False
    else:
        pool, reduced = build_pool(feats, a.max_rows, a.reduce_to, a.seed, a.max_iter, a.tol, **({} if a.metric == "l2" else {"metric": a.metric}))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    index = UnitsIndex(pool, source_rows=feats.shape[0], reduced=reduced, metric=a.metric)
    if a.nlist:
        if not 1 <= a.nlist <= min(65536, pool.shape[0]):
            raise SystemExit(f"--nlist {a.nlist} outside 1 .. min(65536, the pool's {pool.shape[0]} rows)")
        torch.manual_seed(a.seed)
        ck = cluster.train_cluster(pool, a.nlist, max_iter=a.nlist_iter, tol=a.tol, **_mode(a.metric))
        index.build_ivf(a.nlist, centres=np.asarray(ck["cluster_centers_"], dtype=np.float32))
    index.save(a.out)
    print(f"{a.out}: {pool.shape[0]} rows of {pool.shape[1]} floats ({'k-means centres of' if reduced else 'the frames of' if not a.synthetic else 'synthetic, beside'} "
          f"{feats.shape[0]} frames of {min(len(paths), a.max_files)} files)" + (f", {index.nlist} IVF lists" if a.nlist else "") + (f", metric {a.metric}" if a.metric != "l2" else ""))


if __name__ == "__main__":
    main()
