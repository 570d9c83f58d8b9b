"""The XLSR-53 units encoder (wav2vec 2.0, 24 layers at width 1024), seeded weights, one process: B = 1 and B = 8 clips of 480,000
samples, and 8 clips of 8 lengths (5 .. 30 s) as one ragged call against one call per clip; the HuBERT-base and Whisper large-v3 encodes
of the same B = 8 clips measured in the same rounds, the two encoders it stands beside; tools/bench_hubert.py's method: warm-up, device
events around whole calls, alternating rounds, the minimum with the rounds reported; one JSON line.  `--stages` adds the per-launch split
of one B = 8 encode (HIP-event profiler) on stderr, with bytes per launch against the memory rate for the bandwidth-bound ones (w2v_conv0,
w2v_ln_act).

    python tools/bench_xlsr.py [--iters 3] [--warmup 1] [--rounds 3] [--layers 24] [--no-others] [--stages]

FLOP of one clip of n samples (frames n0 .. n6 = T after conv0 .. conv6 without padding; D = 512, C = 1024, F = 4096, K = 128, 64 channels
per group): conv0 2 * 10 * D * n0; conv_i 2 * k_i * D^2 * n_i (k = 3, 3, 3, 3, 2, 2); projection 2 * D * C * T; positional convolution
2 * C * 64 * K * T; per block (2 * (4 C^2 + 2 C F) + 4 T C) * T.  At 480,000 samples (1,499 frames): blocks 0.905 T, attention 0.221 T,
conv stack 0.147 T, positional convolution 0.025 T, projection 0.002 T: 1.30 TFLOP."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "latent-diffusion-speech_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import bench_hubert  # noqa: E402
from lds import arch, init_weights, native  # noqa: E402

PEAK_TFLOPS, PEAK_TBS = bench_hubert.PEAK_TFLOPS, bench_hubert.PEAK_TBS


def flop(n_samples, dims, layers):
    """algorithmic FLOP of one clip (the module docstring's formula) -> (total, parts)"""
    D, C, F, K = dims["conv_dim"], dims["n_state"], dims["n_ffn"], dims["pos_kernel"]
    gw = C // dims["pos_groups"]
    n = arch.hubert_level_frames(n_samples, 0)
    T = n[6]
    parts = {"conv0": 2 * 10 * D * n[0], "conv1_6": sum(2 * (3 if i <= 4 else 2) * D * D * n[i] for i in range(1, 7)),
             "projection": 2 * D * C * T, "posconv": 2 * C * gw * K * T,
             "blocks": layers * 2 * (4 * C * C + 2 * C * F) * T, "attention": layers * 4 * T * C * T}
    return sum(parts.values()), parts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--no-others", action="store_true", help="leave the HuBERT and Whisper legs out")
    ap.add_argument("--stages", action="store_true")
    a = ap.parse_args()
    dims = dict(arch.XLSR_53_DIMS, n_layer=a.layers)
    h = native.Wav2Vec2(dims, arch.w2v_init_state(dims, 0))
    L = 480000
    audio = torch.from_numpy(init_weights.uniform("bench.units.audio", (8, L), 5, -0.5, 0.5)).cuda()
    lens = [80000 + (L - 80000) * i // 7 for i in range(8)]      # 5 .. 30 s
    clips = [audio[b:b + 1, :n].contiguous() for b, n in enumerate(lens)]
    legs = [("b1", lambda: h.encode(audio[:1])), ("b8", lambda: h.encode(audio)), ("rag", lambda: h.encode(audio, lens)),
            ("seq", lambda: [h.encode(c) for c in clips])]
    if not a.no_others:
        hd = dict(arch.HUBERT_BASE_DIMS)
        hub = native.Hubert(hd, arch.hubert_init_state(hd, 0))
        W = bench_hubert
        wh = native.Whisper(W.W_MELS, W.W_C, W.W_HEADS, 32, W.W_CTX, arch.whisper_init_state(W.W_MELS, W.W_C, 32, 0), arch.whisper_mel_filters(W.W_MELS))
        legs += [("hubert_b8", lambda: hub.encode(audio, proj=True)), ("whisper_b8", lambda: wh.encode(audio))]
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
        fh = 8 * bench_hubert.flop(L, arch.HUBERT_BASE_DIMS, 12)[0]
        fw = 8 * bench_hubert.whisper_flop(L, 32)
        out.update({"hubert_b8_ms": round(ms["hubert_b8"], 3), "hubert_b8_tflops": round(fh / ms["hubert_b8"] / 1e9, 1),
                    "whisper_b8_ms": round(ms["whisper_b8"], 3), "whisper_b8_tflops": round(fw / ms["whisper_b8"] / 1e9, 1)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
