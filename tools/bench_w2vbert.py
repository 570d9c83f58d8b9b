"""The w2v-BERT 2.0 units encoder (a Conformer of 24 blocks at width 1024 behind a filter bank), seeded weights, one process: B = 1 and
B = 8 clips of 480,000 samples, and 8 clips of 8 lengths (5 .. 30 s) as one ragged call against one call per clip; the XLSR-53 and Whisper
large-v3 encodes of the same B = 8 clips measured in the same rounds, the two encoders it stands beside; tools/bench_xlsr.py's method:
warm-up, device events around whole calls, alternating rounds, the minimum with the rounds reported; one JSON line.  `--stages` adds the
per-launch split of one B = 8 encode (HIP-event profiler) on stderr, with bytes per launch against the memory rate for the bandwidth-bound
ones (w2vbert_fbank_*, w2vbert_dwconv).

    python tools/bench_w2vbert.py [--iters 3] [--warmup 1] [--rounds 3] [--layers 24] [--no-others] [--stages]

FLOP of one clip of n samples (n frames -> T = ceil(n / 2) rows; M = 80 mel bins, Fd = 160, C = 1024, F = 4096, K = 31 taps, R = 73 distances):
filter bank 2 * 257 * (2 * 400 + M) * n; projection 2 * Fd * C * T; per block the two feed-forwards 2 * 4 C F * T, q | k | v | out 2 * 4 C^2 * T,
the two pointwise convolutions 2 * 3 C^2 * T, the depthwise convolution 2 * K * C * T, the relative-key table 2 * C * R * T and attention
4 T C * T.  At 480,000 samples (2,998 frames, 1,499 rows): blocks 1.73 T, attention 0.22 T, the rest 0.01 T: 1.96 TFLOP."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "latent-diffusion-speech_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import bench_hubert  # noqa: E402
import bench_xlsr  # noqa: E402
from lds import arch, init_weights, native  # noqa: E402

PEAK_TFLOPS, PEAK_TBS = bench_hubert.PEAK_TFLOPS, bench_hubert.PEAK_TBS


def flop(n_samples, dims, layers):
    """algorithmic FLOP of one clip (the module docstring's formula) -> (total, parts)"""
    M, C, F, K = dims["n_mels"], dims["n_state"], dims["n_ffn"], dims["dw_kernel"]
    Fd, R = M * dims["stride"], dims["left_max"] + dims["right_max"] + 1
    n, _, T = arch.w2vbert_frames(n_samples)
    parts = {"fbank": 2 * 257 * (2 * 400 + M) * n, "projection": 2 * Fd * C * T,
             "blocks": layers * (2 * (4 * C * F + 4 * C * C + 3 * C * C) + 2 * K * C + 2 * C * R) * T, "attention": layers * 4 * T * C * T}
    return sum(parts.values()), parts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--no-others", action="store_true", help="leave the XLSR-53 and Whisper legs out")
    ap.add_argument("--stages", action="store_true")
    a = ap.parse_args()
    dims = dict(arch.W2V_BERT_DIMS, n_layer=a.layers)
    h = native.Wav2Vec2Bert(dims, arch.w2vbert_init_state(dims, 0))
    L = 480000
    audio = torch.from_numpy(init_weights.uniform("bench.units.audio", (8, L), 5, -0.5, 0.5)).cuda()
    lens = [80000 + (L - 80000) * i // 7 for i in range(8)]      # 5 .. 30 s
    clips = [audio[b:b + 1, :n].contiguous() for b, n in enumerate(lens)]
    legs = [("b1", lambda: h.encode(audio[:1])), ("b8", lambda: h.encode(audio)), ("rag", lambda: h.encode(audio, lens)),
            ("seq", lambda: [h.encode(c) for c in clips])]
    if not a.no_others:
        xd = dict(arch.XLSR_53_DIMS)
        xl = native.Wav2Vec2(xd, arch.w2v_init_state(xd, 0))
        W = bench_hubert
        wh = native.Whisper(W.W_MELS, W.W_C, W.W_HEADS, 32, W.W_CTX, arch.whisper_init_state(W.W_MELS, W.W_C, 32, 0), arch.whisper_mel_filters(W.W_MELS))
        legs += [("xlsr_b8", lambda: xl.encode(audio)), ("whisper_b8", lambda: wh.encode(audio))]
    for _ in range(a.warmup):
        for _, fn in legs:
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k, _ in legs}
    for _ in range(a.rounds):      # alternating: every leg sees the same clocks and the same neighbours
        for k, fn in legs:
            t[k].append(bench_hubert.timed(fn, a.iters))
    ms = {k: min(v) for k, v in t.items()}
    f1, parts = flop(L, dims, a.layers)
    fr = sum(flop(n, dims, a.layers)[0] for n in lens)
    if a.stages:
        native.prof_enable(2)
        legs[1][1]()
        torch.cuda.synchronize()
        prof = native.prof_summary()
        native.prof_enable(0)
        tot = sum(r["ms"] for r in prof)
        print(f"B = 8 encode, profiled: {tot:.2f} ms in {sum(r['count'] for r in prof)} launches", file=sys.stderr)
        for r in sorted(prof, key=lambda r: -r["ms"]):
            tf = r["flops"] / (r["ms"] * 1e-3) / 1e12 if r["flops"] else 0
            tb = r["bytes"] / (r["ms"] * 1e-3) / 1e12 if r.get("bytes") else 0
            print(f"{r['name']:80s} n={r['count']:3d} {r['ms']:8.3f} ms {100 * r['ms'] / tot:5.1f}% {tf:6.1f} TF ({100 * tf / PEAK_TFLOPS:4.1f}% of peak) "
                  f"{tb:5.2f} TB/s ({100 * tb / PEAK_TBS:4.1f}% of HBM)", file=sys.stderr)
    out = {
        "layers": a.layers, "b1_ms": round(ms["b1"], 3), "b8_ms": round(ms["b8"], 3), "ragged8_ms": round(ms["rag"], 3), "per_clip8_ms": round(ms["seq"], 3),
        "clip_tflop": round(f1 / 1e12, 4), "clip_tflop_parts": {k: round(v / 1e12, 4) for k, v in parts.items()},
        "b8_tflop": round(8 * f1 / 1e12, 3), "ragged8_tflop": round(fr / 1e12, 3),
        "b1_tflops": round(f1 / ms["b1"] / 1e9, 1), "b8_tflops": round(8 * f1 / ms["b8"] / 1e9, 1), "ragged8_tflops": round(fr / ms["rag"] / 1e9, 1),
        "per_clip8_tflops": round(fr / ms["seq"] / 1e9, 1), "b8_frac_peak": round(8 * f1 / ms["b8"] / 1e9 / PEAK_TFLOPS, 3),
        "per_clip_over_ragged": round(ms["seq"] / ms["rag"], 3), "rounds_ms": {k: [round(x, 3) for x in v] for k, v in t.items()},
        "ragged_lengths": lens}
    if not a.no_others:
        fx = 8 * bench_xlsr.flop(L, arch.XLSR_53_DIMS, 24)[0]
        fw = 8 * bench_hubert.whisper_flop(L, 32)
        out.update({"xlsr_b8_ms": round(ms["xlsr_b8"], 3), "xlsr_b8_tflops": round(fx / ms["xlsr_b8"] / 1e9, 1),
                    "whisper_b8_ms": round(ms["whisper_b8"], 3), "whisper_b8_tflops": round(fw / ms["whisper_b8"] / 1e9, 1)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
