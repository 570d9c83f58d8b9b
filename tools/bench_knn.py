"""Units retrieval (cluster.index.UnitsIndex.retrieve: lds_knn_retrieve) at the sizes people use: N = 12,000 query frames (two minutes of
audio), D = 1280, k = 8, against pools of M = 100,000 and 1,000,000 rows; one JSON line, also written to --out.

    python tools/bench_knn.py [--pools 100000 1000000] [--reps 5] [--out profiles/r20_knn_bench.json]

Event time on the stream around one whole call after a warm-up call, the median of --reps.  tflops = 2 N M D / time: a figure for the whole
call (search, merge, gather and blend), to set beside the assign's kernel figures (tools/bench_kmeans.py).  The baseline is the same
computation in torch on the same device: x @ p.T - h in chunks of pool rows with a running topk, then the gather, the distances, the
weights and the blend.  A measurement, not a gate.
"""
import argparse
import json
import os
import statistics
import sys

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
    return statistics.median(t)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_knn_bench.json"))
    a = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(N, D, device="cuda", generator=g)
    res = {"N": N, "D": D, "k": K, "ratio": 0.5, "reps": a.reps, "peak_tflops": PEAK_TFLOPS}
    for M in a.pools:
        p = torch.randn(M, D, device="cuda", generator=g)
        ix = UnitsIndex(p)
        h = ix._device(p.device)[1]
        ms = median_ms(lambda: ix.retrieve(x, k=K, ratio=0.5), a.reps)
        tms = median_ms(lambda: torch_retrieve(x, p, h, K, 0.5), a.reps)
        y, idx, _ = ix.retrieve(x, k=K, ratio=0.5, return_neighbours=True)
        ty, tidx = torch_retrieve(x, p, h, K, 0.5)
        fl = 2.0 * N * M * D
        res[f"retrieve_{M}"] = {"ms": round(ms, 3), "tflops": round(fl / ms / 1e9, 1), "frac_peak": round(fl / ms / 1e9 / PEAK_TFLOPS, 3),
                                "torch_ms": round(tms, 3), "torch_tflops": round(fl / tms / 1e9, 1), "speedup_over_torch": round(tms / ms, 2),
                                "rows_with_torchs_neighbours": round(float((idx == tidx).all(1).float().mean()), 5),
                                "max_abs_y_minus_torch": float((y - ty).abs().max())}
        del p, ix, h
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
