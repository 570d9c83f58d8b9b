"""Generate the k-means tokenizer's golden fixtures (tests/golden/kmeans.npz, manifest_kmeans.json: the reference's signatures as
[name, repr(default)] lists) by running the reference's own code.

Runs ONLY in the build container (needs /root/reference and scikit-learn); the GPU box never sees the reference.  Inputs are
regenerated from seeds by tests/kmeans_numpy.py make_blobs and never stored.  Recorded:

  predict  `cluster.get_cluster_result` (reference cluster/__init__.py:5-18, scikit-learn's predict on a model poured from a checkpoint
           dict) on five cases (CASES below): blobs at K 4096 x D 1280 and K 1000 x D 256, pure N(0, 1) points at 4096 x 1280, one shape
           that is a multiple of no tile, one [B, T, D] ragged case.  Per case: scikit-learn's labels, the float64 arg-min, every row's
           float64 gap between the best and the runner-up squared distance, the seed.  A case is "clear" when scikit-learn's labels equal
           the float64 arg-min on every row and every gap exceeds eps(n) (kmeans_numpy.eps_bound); the recipe re-seeds until that holds
           and asserts it for the four blob cases.  The pure N(0, 1) case has rows whose runner-up lies within eps (no planted partition), so
           it is stored with `clear` = 0: there only scikit-learn's labels = the float64 arg-min is asserted.
  fit      KMeansGPU(device=cpu) (reference cluster/kmeans.py:51-206) with an import-only pynvml placeholder reporting 8 GiB free (full-batch
           mode), K 64 x D 96 x N 6000 blobs, tol 1e-2: the starting centroids (captured from _kpp), every iteration's labels and error, the
           final centroids; and the float64 restatement (kmeans_numpy.fit64) from the same start.  Asserted: same iteration count, the
           same labels in every iteration, no error within 1 % of tol.
  seeding  _kpp (kmeans.py:10-50) on N 512, K 16, D 32 with the draws replayed (torch.manual_seed, one randint, K - 1 Uniform.sample): the
           first index, the uniforms, the reference's picks.  Asserted: the picks equal the float64 running-minimum restatement's and every
           draw is at least max(N, 2 (D + 2)) 2^-24 away from the nearest CDF boundary (rounding cannot move a pick); re-seeded until so.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_kmeans_fixtures.py [--out DIR]
    python tests/golden/make_kmeans_fixtures.py --check      # regenerate into a temporary directory, compare every array bit for bit
"""
import argparse
import importlib.machinery
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.dont_write_bytecode = True

# name: (K, D, N, spread (None = pure N(0,1) points), first seed, B (ragged) or 0, lengths)
CASES = {
    "blobs_4096x1280": (4096, 1280, 3000, 0.5, 100, 0, None),
    "blobs_1000x256": (1000, 256, 3000, 0.5, 200, 0, None),
    "normal_4096x1280": (4096, 1280, 600, None, 300, 0, None),
    "odd_333x136": (333, 136, 1501, 0.5, 400, 0, None),
    "ragged_1000x256": (1000, 256, 150, 0.5, 500, 3, (50, 17, 33)),
}
FIT = dict(K=64, D=96, N=6000, seed=7, tol=1e-2, max_iter=200)
SEED = dict(K=16, D=32, N=512, first_seed=11)


def _load_by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _placeholder(name, **attrs):
    m = types.ModuleType(name)
    m.__spec__ = importlib.machinery.ModuleSpec(name, None)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def generate(out_dir):
    import torch
    kn = _load_by_path("kmeans_numpy", os.path.join(ROOT, "tests", "kmeans_numpy.py"))
    _placeholder("pynvml", nvmlInit=lambda: None, nvmlDeviceGetHandleByIndex=lambda i: None,
                 nvmlDeviceGetMemoryInfo=lambda h: types.SimpleNamespace(free=8 * 1024 ** 3))
    ref_cluster = _load_by_path("ref_cluster", os.path.join(REF, "cluster", "__init__.py"))
    ref_km = _load_by_path("ref_kmeans", os.path.join(REF, "cluster", "kmeans.py"))
    out = {}

    # ---- predict ----
    for name, (K, D, N, spread, seed0, B, lens) in CASES.items():
        for seed in range(seed0, seed0 + 20):
            C, X, _ = kn.make_blobs(seed, K, D, N, spread)
            with tempfile.TemporaryDirectory() as td:
                ck = os.path.join(td, "semantic_codebook.pt")
                torch.save({"n_features_in_": D, "_n_threads": 4, "cluster_centers_": C}, ck)
                real_load = torch.load
                torch.load = lambda p, **kw: real_load(p, weights_only=False, **kw)      # (numpy arrays inside: not a weights-only file)
                try:
                    model = ref_cluster.get_cluster_model(ck)
                finally:
                    torch.load = real_load
            sk = ref_cluster.get_cluster_result(model, X)
            lab, gap = kn.assign64(X, C)
            clear = bool((gap > kn.eps_bound(X, C)).all())
            # (pure N(0, 1) points have no planted partition: a few rows' runners-up sit within eps, so that case cannot be "clear"; it is
            # recorded with clear = 0 and scikit-learn's labels must still equal the float64 arg-min on every row)
            if np.array_equal(sk, lab) and (clear or spread is None):
                break
        else:
            raise AssertionError(f"{name}: no clear seed in 20")
        out[f"{name}.clear"] = np.int64(clear)
        out[f"{name}.seed"], out[f"{name}.shape"] = np.int64(seed), np.array([K, D, N, B], np.int64)
        out[f"{name}.spread"] = np.float64(-1.0 if spread is None else spread)
        out[f"{name}.sk"], out[f"{name}.f64"], out[f"{name}.gap"] = sk.astype(np.int32), lab.astype(np.int32), gap
        if lens is not None:
            out[f"{name}.lengths"] = np.array(lens, np.int32)
        print(f"predict {name}: seed {seed}, min gap / eps {float((gap / kn.eps_bound(X, C)).min()):.3g}")

    # ---- fit ----
    K, D, N, tol = FIT["K"], FIT["D"], FIT["N"], FIT["tol"]
    _, X, _ = kn.make_blobs(FIT["seed"], K, D, N, 0.5)
    cap = {"labels": [], "errors": []}
    real_kpp = ref_km._kpp

    def kpp(*a, **kw):
        cap["start"] = real_kpp(*a, **kw).clone()
        return cap["start"].clone()

    class Loop:
        def __init__(self, it):
            self.it = it

        def __iter__(self):
            return iter(self.it)

        def set_postfix(self, error):
            cap["errors"].append(error)

    ref_km._kpp, ref_km.tqdm = kpp, Loop
    km = ref_km.KMeansGPU(n_clusters=K, mode="euclidean", verbose=0, max_iter=FIT["max_iter"], tol=tol, device=torch.device("cpu"))
    real_max_sim = km.max_sim

    def max_sim(a, b):
        v, i = real_max_sim(a, b)
        cap["labels"].append(i.numpy().copy())
        return v, i

    km.max_sim = max_sim
    torch.manual_seed(FIT["seed"])
    last = km.fit_predict(torch.from_numpy(X))
    ref_km._kpp = real_kpp
    start = cap["start"].numpy()
    f64 = kn.fit64(X, start, FIT["max_iter"], tol)
    n_iter = len(cap["errors"])
    assert n_iter == f64["n_iter"], (n_iter, f64["n_iter"])
    assert all(np.array_equal(a, b) for a, b in zip(cap["labels"], f64["labels"])), "fit: fp32 and float64 labels differ"
    assert np.array_equal(last.numpy().astype(np.int64), cap["labels"][-1])
    errs = np.array(cap["errors"], np.float64)
    assert (np.abs(errs - tol) > 0.01 * tol).all() and (np.abs(f64["errors"] - tol) > 0.01 * tol).all(), "fit: an error within 1 % of tol"
    cref = km.centroids.numpy()
    out["fit.start"], out["fit.labels"] = start, np.stack(cap["labels"]).astype(np.uint8)
    out["fit.errors"], out["fit.errors64"] = errs.astype(np.float32), f64["errors"]
    out["fit.centroids"], out["fit.centroids64"], out["fit.num_points64"] = cref, f64["centroids"], f64["num_points"]
    out["fit.gap"] = np.float64(np.abs(cref - f64["centroids"]).max() / np.abs(f64["centroids"]).max())
    print(f"fit: {n_iter} iterations, fp32 vs float64 centroids {float(out['fit.gap']):.2e} of abs-max")

    # ---- seeding ----
    K, D, N = SEED["K"], SEED["D"], SEED["N"]
    need = max(N, 2 * (D + 2)) * 2.0 ** -24
    for seed in range(SEED["first_seed"], SEED["first_seed"] + 40):
        _, X, _ = kn.make_blobs(seed, K, D, N, 0.5)
        torch.manual_seed(seed)
        first = int(torch.randint(N, [1]))
        r = torch.distributions.uniform.Uniform(0, 1)
        u = np.array([float(r.sample([1])) for _ in range(K - 1)], np.float32)
        torch.manual_seed(seed)
        init = real_kpp(torch.from_numpy(X), K, N).numpy()
        picks = np.array([int(np.flatnonzero((X == row).all(1))[0]) for row in init])
        p64, clear = kn.kpp64(X, K, first, u)
        if np.array_equal(picks, p64) and clear.min() >= need:
            break
    else:
        raise AssertionError("seeding: no seed with the clearance in 40")
    out["seed.seed"], out["seed.first"], out["seed.uniforms"], out["seed.picks"] = np.int64(seed), np.int64(first), u, picks.astype(np.int64)
    out["seed.clearance"] = np.float64(clear.min())
    print(f"seeding: seed {seed}, clearance {clear.min():.2e} (needed {need:.2e})")
    np.savez_compressed(os.path.join(out_dir, "kmeans.npz"), **out)
    import inspect
    import json
    sig = {"KMeansGPU.__init__": ref_km.KMeansGPU.__init__, "KMeansGPU.fit_predict": ref_km.KMeansGPU.fit_predict, "KMeansGPU.max_sim": ref_km.KMeansGPU.max_sim,
           "_kpp": real_kpp, "get_cluster_model": ref_cluster.get_cluster_model, "get_cluster_result": ref_cluster.get_cluster_result,
           "get_cluster_center_result": ref_cluster.get_cluster_center_result, "get_center": ref_cluster.get_center}
    with open(os.path.join(out_dir, "manifest_kmeans.json"), "w") as f:
        json.dump({k: [[n, None if q.default is inspect.Parameter.empty else repr(q.default)] for n, q in inspect.signature(v).parameters.items()]
                   for k, v in sig.items()}, f, indent=1, sort_keys=True)
        f.write("\n")


def check():
    with tempfile.TemporaryDirectory() as td:
        generate(td)
        new, old = np.load(os.path.join(td, "kmeans.npz")), np.load(os.path.join(HERE, "kmeans.npz"))
        assert sorted(new.files) == sorted(old.files), "key sets differ"
        bad = [k for k in old.files if new[k].dtype != old[k].dtype or new[k].tobytes() != old[k].tobytes()]
        assert not bad, f"arrays differ: {bad}"
        assert open(os.path.join(td, "manifest_kmeans.json")).read() == open(os.path.join(HERE, "manifest_kmeans.json")).read(), "manifest differs"
    print("kmeans.npz reproduced bit for bit")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    check() if a.check else generate(a.out)
