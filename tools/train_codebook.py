"""Fit the k-means semantic codebook on unit files (the reference's 17_preprocess_train_cluster.py, its KMeansGPU branch).

    python tools/train_codebook.py UNITS_DIR [--out pretrain/semantic_codebook.pt] [--n_clusters 4096] [--max_files 30000] [--seed 0]
                                   [--max_iter 500] [--tol 1e-2] [--minibatch N]

UNITS_DIR holds .npy unit files [T, dim] (tools/extract_units.py writes them), searched recursively; up to --max_files of them
(shuffled with --seed) are concatenated and clustered by cluster.train_cluster (k-means++ seeding, assignment and Lloyd steps on
the HIP device).  The result is the reference's checkpoint dict, loadable by cluster.get_cluster_model and infer_tts.py --codebook.
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("units_dir")
    ap.add_argument("--out", default="pretrain/semantic_codebook.pt")
    ap.add_argument("--n_clusters", type=int, default=4096)
    ap.add_argument("--max_files", type=int, default=30000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max_iter", type=int, default=500)
    ap.add_argument("--tol", type=float, default=1e-2)
    ap.add_argument("--minibatch", type=int, default=None)
    ap.add_argument("--mode", default="euclidean", choices=("euclidean", "cosine"), help="KMeansGPU's distance measure (extract_tokens.py --metric cosine "
                    "assigns by a cosine codebook)")
    a = ap.parse_args()
    paths = sorted(glob.glob(os.path.join(a.units_dir, "**", "*.npy"), recursive=True))
    if not paths:
        raise SystemExit(f"no .npy unit files under {a.units_dir}")
    random.Random(a.seed).shuffle(paths)
    feats = np.concatenate([np.load(p).astype(np.float32) for p in paths[: a.max_files]], axis=0)
    torch.manual_seed(a.seed)
    kw = {} if a.minibatch is None else {"minibatch": a.minibatch}
    if a.mode != "euclidean":
        kw["mode"] = a.mode
    ck = cluster.train_cluster(feats, a.n_clusters, max_iter=a.max_iter, tol=a.tol, **kw)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    torch.save(ck, a.out)
    print(f"{a.out}: {a.n_clusters} centres of {feats.shape[1]} floats from {feats.shape[0]} frames of {min(len(paths), a.max_files)} files")


if __name__ == "__main__":
    main()
