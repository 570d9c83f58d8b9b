"""Units retrieval (cluster.index.UnitsIndex.retrieve: lds_knn_retrieve) at the sizes people use: N = 12,000 query frames (two minutes of
audio), D = 1280, k = 8, against pools of M = 100,000 and 1,000,000 rows; one JSON line, also written to --out.

    python tools/bench_knn.py [--pools 100000 1000000] [--reps 5] [--out profiles/r20_knn_bench.json]

Event time on the stream around one whole call after a warm-up call, the median of --reps.  tflops = 2 N M D / time: a figure for the whole
call (search, merge, gather and blend), to set beside the assign's kernel figures (tools/bench_kmeans.py).  The baseline is the same
computation in torch on the same device: x @ p.T - h in chunks of pool rows with a running topk, then the gather, the distances, the
weights and the blend.  A measurement, not a gate.

    python tools/bench_knn.py --nlist 256 1024 --nprobe 1 8 [--mixture 256] [--no_torch] [--out profiles/r23_ivf_bench.json]

--nlist / --nprobe: the IVF coarse index (UnitsIndex.build_ivf, retrieve(nprobe=)) beside the exact call of the same session.  Pool and
queries then come from one seeded Gaussian mixture of --mixture components (unit-variance noise around N(0, 4) centres: a plain Gaussian has
no neighbours worth finding at this width).  Per (pool, nlist): the build's wall time (fit + assignment + the list-ordered copy); per nprobe:
the call's median, its ratio to the exact call, the kernels' shares of one profiled call (ivf_scan, the coarse knn_topk, knn_blend) and
recall@8 against the exact call's lists.  exact_ms_spread is (max - min) of the exact call's --reps timings.

    python tools/bench_knn.py --metric l2 cosine [--nlist 1024 --nprobe 8] [--out profiles/r24_cosine_knn_bench.json]

--metric (default l2: everything above, unchanged): one metric runs the figures above on an index of that metric (the torch baseline is
Euclidean and is left out for cosine); two metrics are timed against each other in ALTERNATING rounds in one process -- round r times one
call of each metric in turn, on indexes over the same device pool -- and reported as median and (max - min) per metric, for the exact call and
for every (nlist, nprobe).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "latent-diffusion-speech_amd"))
import torch  # noqa: E402

from cluster.index import UnitsIndex  # noqa: E402

PEAK_TFLOPS = 157.3
N, D, K = 12000, 1280, 8


def median_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1))
    median_ms.last = t
    return statistics.median(t)


def mixture(n, d, comps, centres_seed, seed):
    """n rows around `comps` seeded centres (the same centres for every seed)"""
    c = torch.randn(comps, d, device="cuda", generator=torch.Generator(device="cuda").manual_seed(centres_seed)) * 2.0
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = torch.randn(n, d, device="cuda", generator=g)
    for r in range(0, n, 1 << 18):      # (in pieces: the gathered centres of a million rows are one more pool)
        out[r:r + (1 << 18)] += c[torch.randint(0, comps, (min(1 << 18, n - r),), device="cuda", generator=g)]
    return out


def ivf_figures(ix, x, exact_ms, exact_idx, nlists, nprobes, reps):
    from lds import native
    out = {}
    for nlist in nlists:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ix.build_ivf(nlist)
        ix._device_ivf(x.device)
        torch.cuda.synchronize()
        lens = ix.ivf["offsets"][1:] - ix.ivf["offsets"][:-1]
        res = {"build_s": round(time.perf_counter() - t0, 2), "lists_left": ix.nlist, "copy_rows": int(ix._device_ivf(x.device)[4].shape[0]),
               "list_rows_mean_max": [round(float(lens.mean()), 1), int(lens.max())]}
        for nprobe in nprobes:
            ms = median_ms(lambda: ix.retrieve(x, k=K, ratio=0.5, nprobe=nprobe), reps)
            native.prof_enable(1)
            _, idx, _ = ix.retrieve(x, k=K, ratio=0.5, return_neighbours=True, nprobe=nprobe)
            prof = {r["name"]: r["ms"] for r in native.prof_summary()}
            native.prof_enable(0)
            hit = (idx[:, :, None] == exact_idx[:, None, :]).any(2).float().mean()
            per_list = torch.bincount(ix.probe_lists(x, nprobe).reshape(-1), minlength=ix.nlist)
            res[f"nprobe_{nprobe}"] = {"ms": round(ms, 3), "speedup_over_exact": round(exact_ms / ms, 2), "recall_at_8": round(float(hit), 4),
                                       "queries_per_list_mean_max": [round(float(per_list.float().mean()), 1), int(per_list.max())],
                                       "profiled_ms": {k: round(v, 3) for k, v in prof.items()}}
        out[f"nlist_{nlist}"] = res
    return out


def one_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternating(calls, reps):
    """calls {name: fn}: one warm-up call each, then `reps` rounds of one timed call of each in turn -> {name: {"ms", "spread_ms", "all_ms"}}"""
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    t = {name: [] for name in calls}
    for _ in range(reps):
        for name, fn in calls.items():
            t[name].append(one_ms(fn))
    return {name: {"ms": round(statistics.median(v), 3), "spread_ms": round(max(v) - min(v), 3), "all_ms": [round(q, 3) for q in v]} for name, v in t.items()}


def metric_rounds(a, x, res):
    """--metric with two metrics: the exact call and every (nlist, nprobe) of each metric in alternating rounds over one device pool"""
    for M in a.pools:
        p = mixture(M, D, a.mixture, 1, 3) if a.nlist else torch.randn(M, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(M))
        ixs = {m: UnitsIndex(p, metric=m) for m in a.metric}
        res[f"retrieve_{M}"] = alternating({m: (lambda ix=ix: ix.retrieve(x, k=K, ratio=0.5)) for m, ix in ixs.items()}, a.reps)
        for nlist in a.nlist:
            for ix in ixs.values():
                ix.build_ivf(nlist)
                ix._device_ivf(x.device)
            for nprobe in a.nprobe:
                res.setdefault(f"ivf_{M}", {})[f"nlist_{nlist}_nprobe_{nprobe}"] = alternating(
                    {m: (lambda ix=ix: ix.retrieve(x, k=K, ratio=0.5, nprobe=nprobe)) for m, ix in ixs.items()}, a.reps)
            for ix in ixs.values():
                ix._ivf_on = {}
        del p, ixs


def torch_retrieve(x, p, h, k, ratio, chunk=65536):
    best_v = best_i = None
    for m0 in range(0, p.shape[0], chunk):
        s = x @ p[m0:m0 + chunk].T - h[None, m0:m0 + chunk]
        v, i = s.topk(min(k, s.shape[1]), dim=1)
        i = i + m0
        if best_v is not None:
            v, i = torch.cat([best_v, v], 1), torch.cat([best_i, i], 1)
            v, o = v.topk(k, dim=1)
            i = torch.gather(i, 1, o)
        best_v, best_i = v, i
    rows = p[best_i]
    d = ((x[:, None, :] - rows) ** 2).sum(-1).clamp_min(1e-12)
    w = (1.0 / d) ** 2
    w = w / w.sum(1, keepdim=True)
    return (1.0 - ratio) * x + ratio * (w[:, :, None] * rows).sum(1), best_i


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pools", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="default: profiles/r20_knn_bench.json, with --nlist profiles/r23_ivf_bench.json")
    ap.add_argument("--nlist", type=int, nargs="+", default=[])
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--mixture", type=int, default=256)
    ap.add_argument("--no_torch", action="store_true", help="leave the torch baseline out")
    ap.add_argument("--metric", nargs="+", default=["l2"], choices=("l2", "cosine"), help="one: the index's metric; two: alternating rounds of both")
    a = ap.parse_args()
    if len(a.metric) > 2 or len(set(a.metric)) != len(a.metric):
        raise SystemExit("--metric takes one metric, or l2 and cosine once each")
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "r24_cosine_knn_bench.json" if a.metric != ["l2"] else "r23_ivf_bench.json" if a.nlist else "r20_knn_bench.json")
    if a.metric == ["cosine"]:
        a.no_torch = True
    g = torch.Generator(device="cuda").manual_seed(0)
    x = mixture(N, D, a.mixture, 1, 2) if a.nlist else torch.randn(N, D, device="cuda", generator=g)
    res = {"N": N, "D": D, "k": K, "ratio": 0.5, "reps": a.reps, "peak_tflops": PEAK_TFLOPS}
    if a.nlist:
        res["mixture"] = a.mixture
    if a.metric != ["l2"]:
        res["metric"] = a.metric
    if len(a.metric) == 2:
        metric_rounds(a, x, res)
        a.pools = []
    for M in a.pools:
        p = mixture(M, D, a.mixture, 1, 3) if a.nlist else torch.randn(M, D, device="cuda", generator=g)
        ix = UnitsIndex(p, metric=a.metric[0])
        h = ix._device(p.device)[1]
        ms = median_ms(lambda: ix.retrieve(x, k=K, ratio=0.5), a.reps)
        spread = max(median_ms.last) - min(median_ms.last)
        y, idx, _ = ix.retrieve(x, k=K, ratio=0.5, return_neighbours=True)
        fl = 2.0 * N * M * D
        res[f"retrieve_{M}"] = {"ms": round(ms, 3), "tflops": round(fl / ms / 1e9, 1), "frac_peak": round(fl / ms / 1e9 / PEAK_TFLOPS, 3)}
        if not a.no_torch:
            tms = median_ms(lambda: torch_retrieve(x, p, h, K, 0.5), a.reps)
            ty, tidx = torch_retrieve(x, p, h, K, 0.5)
            res[f"retrieve_{M}"].update({"torch_ms": round(tms, 3), "torch_tflops": round(fl / tms / 1e9, 1), "speedup_over_torch": round(tms / ms, 2),
                                         "rows_with_torchs_neighbours": round(float((idx == tidx).all(1).float().mean()), 5),
                                         "max_abs_y_minus_torch": float((y - ty).abs().max())})
            del ty, tidx
        if a.nlist:
            res[f"retrieve_{M}"]["exact_ms_spread"] = round(spread, 3)
            res[f"ivf_{M}"] = ivf_figures(ix, x, ms, idx, a.nlist, a.nprobe, a.reps)
        del p, ix, h
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
