"""Generate the cosine metric's golden fixture (tests/golden/kmeans_cosine.npz) by running the reference's own KMeansGPU(mode="cosine").

Runs ONLY where the reference checkout is (the path make_kmeans_fixtures.py names); the GPU box never sees the reference.  Inputs are
regenerated from seeds by tests/cosine_numpy.py scaled_blobs and never stored; data only goes into the fixture.  Recorded:

  max_sim  KMeansGPU(mode="cosine", device=cpu).max_sim (reference cluster/kmeans.py:96-105 cos_sim, :117-131) on the scaled-blob cases of
           cosine_numpy.BLOBS: K 1000 x D 256 x N 3000, K 333 x D 136 x N 1501 and one ragged case [3, 50, 256] with lengths 50 / 17 / 33.  Per
           case: the reference's labels and similarities, the float64 arg-max, every row's float64 gap between the best and the runner-up
           similarity, the seed, and how many Euclidean labels (kmeans_numpy.assign64) differ from the cosine ones.  A case is "clear" when
           the reference's labels equal the float64 arg-max on every row and every gap exceeds cosine_numpy.search_bound(D); the recipe
           re-seeds until that holds and asserts it.
  fit      KMeansGPU(mode="cosine", device=cpu).fit_predict with the import-only pynvml placeholder of make_kmeans_fixtures.py (8 GiB free:
           full-batch mode) on K 64 x D 96 x N 6000 scaled blobs, tol 1e-2: the starting centroids (captured from _kpp), every iteration's
           labels and error, the final centroids; and the float64 restatement (cosine_numpy.fit64) from the same start.  Asserted: same
           iteration count, the same labels in every iteration, no error within 1 % of tol.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_cosine_fixtures.py [--out DIR]
    python tests/golden/make_cosine_fixtures.py --check      # regenerate into a temporary directory, compare every array bit for bit
"""
import argparse
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
NAME = "kmeans_cosine.npz"


def _by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def generate(out_dir):
    import torch
    mk = _by_path("make_kmeans_fixtures", os.path.join(HERE, "make_kmeans_fixtures.py"))      # (its placeholder, its loader, its reference path)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cosine_numpy as CN
    import kmeans_numpy as KM
    mk._placeholder("pynvml", nvmlInit=lambda: None, nvmlDeviceGetHandleByIndex=lambda i: None,
                    nvmlDeviceGetMemoryInfo=lambda h: types.SimpleNamespace(free=8 * 1024 ** 3))
    ref_km = mk._load_by_path("ref_kmeans", os.path.join(mk.REF, "cluster", "kmeans.py"))
    cpu = torch.device("cpu")
    out = {}

    # ---- max_sim ----
    for name, (K, D, N, seed0, B, lens) in CN.BLOBS.items():
        bound = CN.search_bound(D)
        for seed in range(seed0, seed0 + 20):
            C, X, _ = CN.scaled_blobs(seed, K, D, N)
            km = ref_km.KMeansGPU(n_clusters=K, mode="cosine", device=cpu)
            xin = torch.from_numpy(X.reshape(B, N // B, D) if B else X)
            v, i = km.max_sim(a=xin, b=torch.from_numpy(C))
            ref_lab, ref_sim = i.numpy().reshape(-1), v.numpy().reshape(-1)
            lab, best, gap = CN.assign64(X, C)
            if np.array_equal(ref_lab, lab) and (gap > bound).all():
                break
        else:
            raise AssertionError(f"{name}: no clear seed in 20")
        assert np.abs(ref_sim - best).max() <= CN.sim_bound(D), name
        euc = KM.assign64(X, C)[0]
        out[f"{name}.seed"], out[f"{name}.shape"] = np.int64(seed), np.array([K, D, N, B], np.int64)
        out[f"{name}.ref"], out[f"{name}.f64"], out[f"{name}.gap"] = ref_lab.astype(np.int32), lab.astype(np.int32), gap
        out[f"{name}.ref_sim"], out[f"{name}.euclidean_differs"] = ref_sim.astype(np.float32), np.int64((euc != lab).sum())
        if lens is not None:
            out[f"{name}.lengths"] = np.array(lens, np.int32)
        print(f"max_sim {name}: seed {seed}, min gap {gap.min():.3g} (bound {bound:.3g}), Euclidean labels that differ {int((euc != lab).sum())} of {N}")

    # ---- fit ----
    F = CN.FIT
    K, D, N, tol = F["K"], F["D"], F["N"], F["tol"]
    _, X, _ = CN.scaled_blobs(F["seed"], K, D, N)
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
    km = ref_km.KMeansGPU(n_clusters=K, mode="cosine", verbose=0, max_iter=F["max_iter"], tol=tol, device=cpu)
    real_max_sim = km.max_sim

    def max_sim(a, b):
        v, i = real_max_sim(a, b)
        cap["labels"].append(i.numpy().copy())
        return v, i

    km.max_sim = max_sim
    torch.manual_seed(F["seed"])
    last = km.fit_predict(torch.from_numpy(X))
    ref_km._kpp = real_kpp
    start = cap["start"].numpy()
    f64 = CN.fit64(X, start, F["max_iter"], tol)
    n_iter = len(cap["errors"])
    assert n_iter == f64["n_iter"], (n_iter, f64["n_iter"])
    assert all(np.array_equal(a, b) for a, b in zip(cap["labels"], f64["labels"])), "fit: fp32 and float64 labels differ"
    assert np.array_equal(last.numpy().astype(np.int64), cap["labels"][-1])
    errs = np.array(cap["errors"], np.float64)
    assert (np.abs(errs - tol) > 0.01 * tol).all() and (np.abs(f64["errors"] - tol) > 0.01 * tol).all(), "fit: an error within 1 % of tol"
    gaps = np.array([CN.assign64(X, c)[2].min() for c in [start]])
    cref = km.centroids.numpy()
    out["fit.start"], out["fit.labels"] = start, np.stack(cap["labels"]).astype(np.uint8)
    out["fit.errors"], out["fit.errors64"] = errs.astype(np.float32), f64["errors"]
    out["fit.centroids"], out["fit.centroids64"], out["fit.num_points64"] = cref, f64["centroids"], f64["num_points"]
    out["fit.gap"] = np.float64(np.abs(cref - f64["centroids"]).max() / np.abs(f64["centroids"]).max())
    out["fit.first_gap"] = np.float64(gaps[0])
    print(f"fit: {n_iter} iterations, fp32 vs float64 centroids {float(out['fit.gap']):.2e} of abs-max, first iteration's smallest gap {gaps[0]:.3g}")
    np.savez_compressed(os.path.join(out_dir, NAME), **out)


def check():
    with tempfile.TemporaryDirectory() as td:
        generate(td)
        new, old = np.load(os.path.join(td, NAME)), np.load(os.path.join(HERE, NAME))
        assert sorted(new.files) == sorted(old.files), "key sets differ"
        bad = [k for k in old.files if new[k].dtype != old[k].dtype or new[k].tobytes() != old[k].tobytes()]
        assert not bad, f"arrays differ: {bad}"
    print(f"{NAME} reproduced bit for bit")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    check() if a.check else generate(a.out)
