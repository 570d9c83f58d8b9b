"""The k-means tokenizer without a GPU: the float64 restatement (tests/kmeans_numpy.py) against the reference's recorded results
(tests/golden/kmeans.npz), the C symbols, the reference's signatures, every argument limit through the host-only sanitizer build, and the
refusals of the Python surface (CPU tensors, cosine mode)."""
import glob
import inspect
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import kmeans_numpy as KN
from conftest import GOLDEN, PKG, ROOT

NAMES = ["lds_kmeans_workspace_bytes", "lds_kmeans_prepare", "lds_kmeans_assign", "lds_kmeans_assign_ragged", "lds_kmeans_update", "lds_kmeans_seed"]
FIT = dict(K=64, D=96, N=6000, seed=7, tol=1e-2, max_iter=200)


@pytest.fixture(scope="module")
def fx(golden):
    return golden("kmeans.npz")


@pytest.mark.parametrize("name", ["blobs_4096x1280", "blobs_1000x256", "normal_4096x1280", "odd_333x136", "ragged_1000x256"])
def test_restatement_predict_vs_reference(fx, name):
    K, D, N, B = (int(v) for v in fx[name + ".shape"])
    sp = float(fx[name + ".spread"])
    C, X, _ = KN.make_blobs(int(fx[name + ".seed"]), K, D, N, None if sp < 0 else sp)
    lab, gap = KN.assign64(X, C)
    assert np.array_equal(lab, fx[name + ".sk"]) and np.array_equal(lab, fx[name + ".f64"]) and np.array_equal(gap, fx[name + ".gap"])
    assert bool((gap > KN.eps_bound(X, C)).all()) == bool(fx[name + ".clear"])
    assert (KN.excess64(X, C, lab) == 0).all()


def test_restatement_fit_vs_reference(fx):
    X = KN.make_blobs(FIT["seed"], FIT["K"], FIT["D"], FIT["N"], 0.5)[1]
    r = KN.fit64(X, fx["fit.start"], FIT["max_iter"], FIT["tol"])
    assert r["n_iter"] == len(fx["fit.errors"]) == len(fx["fit.labels"])
    assert all(np.array_equal(a, b) for a, b in zip(r["labels"], fx["fit.labels"].astype(np.int64)))
    assert np.abs(r["errors"] - fx["fit.errors"]).max() / r["errors"].max() < 1e-5      # the reference's fp32 errors
    assert np.abs(r["centroids"] - fx["fit.centroids"]).max() / np.abs(r["centroids"]).max() < 2e-6      # the reference's fp32 centroids
    assert (np.abs(r["errors"] - FIT["tol"]) > 0.01 * FIT["tol"]).all()


def test_restatement_seeding_vs_reference(fx):
    X = KN.make_blobs(int(fx["seed.seed"]), 16, 32, 512, 0.5)[1]
    picks, clear = KN.kpp64(X, 16, int(fx["seed.first"]), fx["seed.uniforms"])
    assert np.array_equal(picks, fx["seed.picks"]) and clear.min() >= max(512, 2 * 34) * 2.0 ** -24
    cum = KN.kpp_interval(X, picks[:5])
    assert (cum[picks[5] - 1] if picks[5] else 0.0) < fx["seed.uniforms"][4] <= cum[picks[5]]


def test_kmeans_symbols_declared_and_exported():
    from lds import native
    hdr = open(os.path.join(ROOT, "include", "lds.h")).read()
    for n in NAMES:
        assert re.search(r"\b" + n + r"\(", hdr), n
    assert "cluster/kmeans.py:10-50" in hdr and "cluster/__init__.py:13-23" in hdr      # the entries cite the lines they replace
    assert set(NAMES) <= set(native.EXPORTS)
    assert os.path.exists(native.LIB_PATH), "liblds.so is not built"
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(NAMES) <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def _params(fn):
    return [[n, None if q.default is inspect.Parameter.empty else repr(q.default)] for n, q in inspect.signature(fn).parameters.items()]


def test_signatures_equal_the_references():
    import cluster
    from cluster.kmeans import KMeansGPU, _kpp
    ref = json.load(open(os.path.join(GOLDEN, "manifest_kmeans.json")))
    got = _params(KMeansGPU.__init__)
    n = len(ref["KMeansGPU.__init__"])
    assert got[:n] == ref["KMeansGPU.__init__"] and [g[0] for g in got[n:]] == ["minibatch", "init"]
    assert all(q.kind is inspect.Parameter.KEYWORD_ONLY for q in list(inspect.signature(KMeansGPU.__init__).parameters.values())[n:])
    assert _params(KMeansGPU.fit_predict) == ref["KMeansGPU.fit_predict"] and _params(KMeansGPU.max_sim) == ref["KMeansGPU.max_sim"]
    assert _params(_kpp) == ref["_kpp"]
    for fn in ("get_cluster_model", "get_cluster_center_result", "get_center"):
        assert _params(getattr(cluster, fn)) == ref[fn], fn
    got = _params(cluster.get_cluster_result)      # the reference's two, then defaulted extras
    assert got[:2] == ref["get_cluster_result"] and all(d is not None for _, d in got[2:])
    assert [p for p, _ in _params(cluster.train_cluster)][:2] == ["features", "n_clusters"]


def test_cpu_tensors_and_cosine_raise():
    import types

    import torch

    import cluster
    from cluster.kmeans import KMeansGPU
    from lds import native
    with pytest.raises(NotImplementedError, match="cosine"):
        KMeansGPU(8, mode="cosine")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KMeansGPU(8, device=torch.device("cpu"))
    x, c = torch.zeros(4, 16), torch.zeros(2, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        native.kmeans_prepare(c)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        native.kmeans_assign(x, c, torch.zeros(2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        native.kmeans_update(x, torch.zeros(4, dtype=torch.int64), c, torch.zeros(2), torch.ones(2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        native.kmeans_seed(x, 2, 0, torch.zeros(1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cluster.get_cluster_result(types.SimpleNamespace(cluster_centers_=np.zeros((2, 16), np.float32)), x)
    with pytest.raises(ValueError, match="codebook"):
        native.kmeans_assign(torch.zeros(4, 8), c, torch.zeros(2))
    with pytest.raises(ValueError, match="device path"):
        cluster.get_cluster_result(types.SimpleNamespace(cluster_centers_=np.zeros((2, 16), np.float32)), np.zeros((4, 16), np.float32), lengths=[4])


DRIVER = r'''
import ctypes as C, sys
sys.path.insert(0, {pkg!r})
from lds import native
native.LIB_PATH = {lib!r}
L = native.lib()
def err():
    return L.lds_last_error().decode()
nb = C.c_size_t()
assert L.lds_kmeans_workspace_bytes(12000, 4096, 1280, C.byref(nb)) == 0 and nb.value > 0
assert L.lds_kmeans_workspace_bytes(2000000, 65536, 4096, C.byref(nb)) == 0 and nb.value > 2000000 * 4
assert L.lds_kmeans_workspace_bytes(12000, 4096, 1280, None) == -1
for N, K, D, bad in ((0, 8, 8, "N 0"), (-5, 8, 8, "N -5"), (1 << 31, 8, 8, "N 2147483648"), (10, 0, 8, "K 0"), (10, 65537, 8, "K 65537"), (10, 8, 0, "D 0"),
                     (10, 8, 4, "D 4"), (10, 8, 12, "D 12"), (10, 8, 4104, "D 4104"), (10, 8, -8, "D -8")):
    assert L.lds_kmeans_workspace_bytes(N, K, D, C.byref(nb)) == -1 and bad in err(), (N, K, D, err())
d = (C.c_float * 64)()      # never touched: every refusal below comes before anything is read or enqueued
i64 = (C.c_int64 * 8)()
ws = (C.c_char * 4096)()
assert L.lds_kmeans_workspace_bytes(100, 16, 64, C.byref(nb)) == 0
big, small = C.c_size_t(nb.value), C.c_size_t(nb.value - 1)
A = lambda **k: dict(dict(X=d, N=100, C_=d, h=d, K=16, D=64, lab=i64, best=d, ws=ws, n=big), **k)
def assign(a):
    return L.lds_kmeans_assign(a["X"], a["N"], a["C_"], a["h"], a["K"], a["D"], a["lab"], a["best"], a["ws"], a["n"], None)
def update(a):
    return L.lds_kmeans_update(a["X"], a["lab"], a["N"], a["C_"], a["h"], a.get("np", d), a["K"], a["D"], a.get("e", d), a["ws"], a["n"], None)
def seed(a):
    return L.lds_kmeans_seed(a["X"], a["N"], a["D"], a["K"], a.get("first", 0), a.get("u", d), a["C_"], a.get("picked", i64), a["ws"], a["n"], None)
for fn in (assign, update, seed):
    for k, bad in ((dict(N=0), "N 0"), (dict(K=0), "K 0"), (dict(K=65537), "K 65537"), (dict(D=4), "D 4"), (dict(D=68), "D 68"), (dict(D=4104), "D 4104")):
        assert fn(A(**k)) == -1 and bad in err(), (fn.__name__, k, err())
    for k in (dict(X=None), dict(C_=None), dict(ws=None)):
        assert fn(A(**k)) == -1 and "null" in err(), (fn.__name__, k, err())
    assert fn(A(n=small)) == -2 and "workspace" in err(), (fn.__name__, err())
for k in (dict(h=None), dict(lab=None)):
    assert assign(A(**k)) == -1 and update(A(**k)) == -1
assert update(A(np=None)) == -1 and update(A(e=None)) == -1
assert seed(A(K=101)) == -1 and "K 101 > N 100" in err()
assert seed(A(first=100)) == -1 and seed(A(first=-1)) == -1 and "first_index" in err()
assert seed(A(u=None)) == -1
assert L.lds_kmeans_prepare(None, 16, 64, d, None) == -1 and L.lds_kmeans_prepare(d, 16, 64, None, None) == -1
assert L.lds_kmeans_prepare(d, 16, 60, d, None) == -1 and "D 60" in err()
lens = (C.c_int32 * 65)(*([5] * 65))
def ragged(B=4, T=25, ln=lens, pad=-1, **k):
    a = A(**k)
    return L.lds_kmeans_assign_ragged(a["X"], B, T, ln, pad, a["C_"], a["h"], a["K"], a["D"], a["lab"], a["best"], a["ws"], a["n"], None)
assert ragged(B=0) == -1 and ragged(B=65) == -1 and "1 .. 64" in err()
assert ragged(T=0) == -1 and ragged(ln=None) == -1 and "lengths" in err()
assert ragged(pad=1 << 40) == -1 and "32 bits" in err()
assert ragged(ln=(C.c_int32 * 4)(5, 26, 5, 5)) == -1 and "lengths[1] = 26" in err()
assert ragged(ln=(C.c_int32 * 4)(5, 5, -1, 5)) == -1 and "lengths[2] = -1" in err()
assert ragged(D=4) == -1 and ragged(X=None) == -1 and ragged(n=small) == -2
print("kmeans driver ok")
'''


def test_kmeans_c_entry_validation_under_asan_ubsan():
    csrc = os.path.join(PKG, "csrc")
    r = subprocess.run(["make", "-C", csrc, "-j", "8", "asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lib = os.path.join(csrc, "build_asan", "liblds_host_asan.so")
    rt = sorted(glob.glob("/opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.asan-x86_64.so"))
    assert rt, "the sanitizer runtime of the ROCm clang is missing"
    env = dict(os.environ, LD_PRELOAD=rt[-1], ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1",
               PYTHONDONTWRITEBYTECODE="1")
    p = subprocess.run([sys.executable, "-c", DRIVER.format(pkg=PKG, lib=lib)], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0 and "kmeans driver ok" in p.stdout, (p.returncode, p.stdout[-1500:], p.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr, p.stderr[-4000:]
