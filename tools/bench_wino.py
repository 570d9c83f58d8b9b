"""Direct (gn_stream + conv_dma) against Winograd F(2,3) (gn_wino + conv_wino) on the resnets' k 3 convolutions, one shape at a time at the
nominal batch, alternating in one process (include/lds_test.h lds_bench_wino):
    python tools/bench_wino.py [--cfgs 0,322,162] [--filter 256] [--json wino_shapes.json]
A shape is routed to conv_wino (csrc/model.hip wino_routed) only where Winograd's mean is lower than the direct pair's by more than the larger
of the two min-max spreads.  cfg = BK * 10 + NST of conv_wino's ring (0 = the launcher's choice by the grid at the nominal batch).
    python tools/bench_wino.py --pair --iters 200 [--json wino_pair_shapes.json]
measures the resnets' conv2 + shortcut tails instead: the direct one (conv_dma_pair) against one conv_wino launch over Cm + Cin / 2 channels
(lds_bench_wino_pair, csrc/model.hip wino_pair_min_T), under the same rule."""
import argparse
import ctypes as ct
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "latent-diffusion-speech_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lds import native  # noqa: E402

# (C1, C2, Co, T, role): every distinct resnet convolution of the UNet at 512 frames that run_resnet could route -- conv1 (no residual, no
# scale / shift; two sources in the up path) and the conv2 of resnets without a shortcut (residual, scale / shift) -- and the level-0 shapes
# at the lengths of the whole-UNet tests
SHAPES = [
    (256, 0, 256, 512, "conv1"), (256, 0, 256, 512, "conv2"), (256, 0, 384, 256, "conv1"), (384, 0, 384, 256, "conv1"), (384, 0, 384, 256, "conv2"),
    (384, 0, 512, 128, "conv1"), (512, 0, 512, 128, "conv1"), (512, 0, 512, 128, "conv2"), (512, 0, 512, 64, "conv1"), (512, 0, 512, 64, "conv2"),
    (512, 512, 512, 64, "conv1"), (512, 512, 512, 128, "conv1"), (512, 384, 512, 128, "conv1"), (512, 384, 384, 256, "conv1"),
    (384, 384, 384, 256, "conv1"), (384, 256, 384, 256, "conv1"), (384, 256, 256, 512, "conv1"), (256, 256, 256, 512, "conv1"),
    (256, 0, 256, 130, "conv1"), (256, 0, 256, 64, "conv1"), (256, 0, 256, 130, "conv2"), (256, 0, 256, 64, "conv2"),
    (384, 256, 256, 130, "conv1"), (256, 256, 256, 64, "conv1"),
]


# --pair: (C1, C2, Cm, T) of the 14 resnets with a shortcut at 512 frames, in the order they run (conv2 + shortcut as one conv_wino launch over
# Cm + Cin / 2 channels, include/lds_test.h lds_bench_wino_pair; both sides include conv1's GroupNorm pass, the new one with its side output)
PAIR_SHAPES = [
    (256, 0, 384, 256), (384, 0, 512, 128), (512, 512, 512, 64), (512, 512, 512, 64), (512, 512, 512, 64), (512, 512, 512, 128), (512, 512, 512, 128),
    (512, 384, 512, 128), (512, 384, 384, 256), (384, 384, 384, 256), (384, 256, 384, 256), (384, 256, 256, 512), (256, 256, 256, 512), (256, 256, 256, 512),
]


def bench_pairs(args, L, rng):
    B, rows = args.B, []
    dp = lambda t: None if t is None else ct.c_void_p(t.data_ptr())      # noqa: E731
    hp = lambda h: ct.c_void_p(h.ctypes.data)      # noqa: E731
    for n, (C1, C2, Cm, T) in enumerate(PAIR_SHAPES):
        name = f"#{n} {C1}+{C2}->{Cm}@{T} pair"
        if args.filter and args.filter not in name:
            continue
        Cin = C1 + C2
        h = torch.from_numpy(rng.standard_normal((B, Cm, T), dtype=np.float32)).cuda()
        x1 = torch.from_numpy(rng.standard_normal((B, C1, T), dtype=np.float32)).cuda()
        x2 = torch.from_numpy(rng.standard_normal((B, C2, T), dtype=np.float32)).cuda() if C2 else None
        ss = torch.from_numpy(0.1 * rng.standard_normal((B, 2 * Cm), dtype=np.float32)).cuda()
        w2 = (rng.standard_normal((Cm, Cm, 3), dtype=np.float32) / np.float32(np.sqrt(3 * Cm))).astype(np.float32)
        ws = (rng.standard_normal((Cm, Cin), dtype=np.float32) / np.float32(np.sqrt(Cin))).astype(np.float32)
        b2, bs = rng.standard_normal((Cm,), dtype=np.float32), rng.standard_normal((Cm,), dtype=np.float32)
        g1, be1, g2, be2 = np.ones(Cin, dtype=np.float32), np.zeros(Cin, dtype=np.float32), np.ones(Cm, dtype=np.float32), np.zeros(Cm, dtype=np.float32)
        for cfg in [int(c) for c in args.cfgs.split(",")]:
            md, mw = (ct.c_float * args.reps)(), (ct.c_float * args.reps)()
            cs = ct.create_string_buffer(256)
            native.check(L.lds_bench_wino_pair(dp(h), dp(x1), dp(x2), Cm, C1, C2, T, hp(g1), hp(be1), hp(g2), hp(be2), dp(ss), 8, hp(w2), hp(b2), hp(ws), hp(bs), cfg,
                                               B, args.iters, args.reps, md, mw, cs, 256, ct.c_void_p(torch.cuda.current_stream().cuda_stream)))
            d, v = np.array(md[:]) * 1e3, np.array(mw[:]) * 1e3      # microseconds per resnet tail (conv1's pass, conv2's pass, the launch)
            gap, spread = d.mean() - v.mean(), max(d.max() - d.min(), v.max() - v.min())
            rows.append(dict(shape=name, Cin=Cin, Cm=Cm, T=T, role="pair", B=B, cfg=cfg, config=cs.value.decode(), direct_us_mean=float(d.mean()),
                             direct_us_min=float(d.min()), direct_us_max=float(d.max()), wino_us_mean=float(v.mean()), wino_us_min=float(v.min()),
                             wino_us_max=float(v.max()), gap_us=float(gap), larger_spread_us=float(spread), wino_faster=bool(gap > spread)))
            print(f"{name:32s} cfg {cfg}  direct {d.mean():7.2f} us [{d.min():.2f}, {d.max():.2f}]  wino {v.mean():7.2f} us [{v.min():.2f}, {v.max():.2f}]"
                  f"  gap {gap:6.2f}  spread {spread:5.2f}  {'WINO' if gap > spread else '-'}", flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfgs", default="0")
    ap.add_argument("--filter", default="")
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default="")
    ap.add_argument("--pair", action="store_true", help="the conv2 + shortcut pairs instead of the single convolutions")
    args = ap.parse_args()
    L = native.lib()
    B = args.B
    rng = np.random.default_rng(0)
    rows = []
    if args.pair:
        rows = bench_pairs(args, L, rng)
    for C1, C2, Co, T, role in ([] if args.pair else SHAPES):
        name = f"{C1}+{C2}->{Co}@{T} {role}"
        if args.filter and args.filter not in name:
            continue
        Ci = C1 + C2
        x1 = torch.from_numpy(rng.standard_normal((B, C1, T), dtype=np.float32)).cuda()
        x2 = torch.from_numpy(rng.standard_normal((B, C2, T), dtype=np.float32)).cuda() if C2 else None
        res = torch.from_numpy(rng.standard_normal((B, Co, T), dtype=np.float32)).cuda() if role == "conv2" else None
        ss = torch.from_numpy(0.1 * rng.standard_normal((B, 2 * Ci), dtype=np.float32)).cuda() if role == "conv2" else None
        w = (rng.standard_normal((Co, Ci, 3), dtype=np.float32) / np.float32(np.sqrt(3 * Ci))).astype(np.float32)
        bias = rng.standard_normal((Co,), dtype=np.float32)
        gamma, beta = np.ones(Ci, dtype=np.float32), np.zeros(Ci, dtype=np.float32)
        for cfg in [int(c) for c in args.cfgs.split(",")]:
            md, mw = (ct.c_float * args.reps)(), (ct.c_float * args.reps)()
            cs = ct.create_string_buffer(256)
            dp = lambda t: None if t is None else ct.c_void_p(t.data_ptr())      # noqa: E731
            hp = lambda h: ct.c_void_p(h.ctypes.data)      # noqa: E731
            native.check(L.lds_bench_wino(dp(x1), dp(x2), C1, C2, T, hp(gamma), hp(beta), dp(ss), 8, 1, hp(w), hp(bias), Co, dp(res), cfg, B, args.iters,
                                          args.reps, md, mw, cs, 256, ct.c_void_p(torch.cuda.current_stream().cuda_stream)))
            d, v = np.array(md[:]) * 1e3, np.array(mw[:]) * 1e3      # microseconds per (GroupNorm pass + convolution)
            gap, spread = d.mean() - v.mean(), max(d.max() - d.min(), v.max() - v.min())
            row = dict(shape=name, Ci=Ci, Co=Co, T=T, role=role, B=B, cfg=cfg, config=cs.value.decode(), direct_us_mean=float(d.mean()), direct_us_min=float(d.min()),
                       direct_us_max=float(d.max()), wino_us_mean=float(v.mean()), wino_us_min=float(v.min()), wino_us_max=float(v.max()),
                       gap_us=float(gap), larger_spread_us=float(spread), wino_faster=bool(gap > spread))
            rows.append(row)
            print(f"{name:28s} cfg {cfg}  direct {d.mean():7.2f} us [{d.min():.2f}, {d.max():.2f}]  wino {v.mean():7.2f} us [{v.min():.2f}, {v.max():.2f}]"
                  f"  gap {gap:6.2f}  spread {spread:5.2f}  {'WINO' if gap > spread else '-'}", flush=True)
    if args.json:
        os.makedirs(os.path.dirname(args.json) or ".", exist_ok=True)
        json.dump(rows, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
