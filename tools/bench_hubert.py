"""The HuBERT units encoder at HuBERT-base's dims, 12 layers, seeded weights, one process: B = 1 and B = 8 clips of 480,000 samples, and 8
clips of 8 lengths (5 .. 30 s) as one ragged call against one call per clip; the Whisper large-v3 encode of the same B = 8 clips for
scale; warm-up, device events around whole calls, alternating rounds, the minimum with the rounds reported; one JSON line.  `--stages`
adds the per-launch split of one B = 8 encode (HIP-event profiler) on stderr, with bytes per launch against the memory rate for the
bandwidth-bound ones (conv0 / norm0, the LayerNorm applications, the frame-major store).

    python tools/bench_hubert.py [--iters 3] [--warmup 1] [--rounds 3] [--layers 12] [--whisper-layers 32] [--no-whisper] [--stages]

FLOP of one clip of n samples (frames n0 .. n6 = T after conv0 .. conv6; D = 512, C = 768, F = 3072, P = 256, K = 128, 48 channels per
group): conv0 2 * 10 * D * n0; conv_i 2 * k_i * D^2 * n_i (k = 3, 3, 3, 3, 2, 2); projection 2 * D * C * T; positional convolution
2 * C * 48 * K * T; per block (2 * (4 C^2 + 2 C F) + 4 T C) * T; proj 2 * C * P * T.  At 480,000 samples: conv stack 0.147 T (conv1 75 G,
conv2 38 G, conv3 19 G, conv4 9 G, conv5..6 5 G, conv0 1 G), blocks 0.255 T, attention 0.083 T, positional convolution 0.014 T, projections
0.002 T: 0.50 TFLOP, against Whisper large-v3's 2.27."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "latent-diffusion-speech_amd"))
import torch  # noqa: E402

from lds import arch, init_weights, native  # noqa: E402

PEAK_TFLOPS = 157.3            # fp32 MFMA peak of the MI355X
PEAK_TBS = 8.0                 # HBM3E rate of the MI355X, TB/s
W_C, W_HEADS, W_MELS, W_CTX = 1280, 20, 128, 1500


def flop(n_samples, dims, layers):
    """algorithmic FLOP of one clip (the module docstring's formula) -> (total, parts)"""
    D, C, F, P, K = dims["conv_dim"], dims["n_state"], dims["n_ffn"], dims["n_proj"], dims["pos_kernel"]
    gw = C // dims["pos_groups"]
    n = arch.hubert_level_frames(n_samples)
    T = n[6]
    parts = {"conv0": 2 * 10 * D * n[0], "conv1_6": sum(2 * (3 if i <= 4 else 2) * D * D * n[i] for i in range(1, 7)),
             "projections": 2 * D * C * T + 2 * C * P * T, "posconv": 2 * C * gw * K * T,
             "blocks": layers * 2 * (4 * C * C + 2 * C * F) * T, "attention": layers * 4 * T * C * T}
    return sum(parts.values()), parts


def whisper_flop(n_samples, layers):
    F = n_samples // 160
    T = (F - 1) // 2 + 1
    return layers * T * (2 * 12 * W_C * W_C + 4 * T * W_C) + F * 2 * 3 * W_MELS * W_C + T * 2 * 3 * W_C * W_C


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--whisper-layers", type=int, default=32)
    ap.add_argument("--no-whisper", action="store_true")
    ap.add_argument("--stages", action="store_true")
    a = ap.parse_args()
    dims = dict(arch.HUBERT_BASE_DIMS, n_layer=a.layers)
    h = native.Hubert(dims, arch.hubert_init_state(dims, 0))
    L = 480000
    audio = torch.from_numpy(init_weights.uniform("bench.units.audio", (8, L), 5, -0.5, 0.5)).cuda()
    lens = [80000 + (L - 80000) * i // 7 for i in range(8)]      # 5 .. 30 s
    clips = [audio[b:b + 1, :n].contiguous() for b, n in enumerate(lens)]
    legs = [("b1", lambda: h.encode(audio[:1], proj=True)), ("b8", lambda: h.encode(audio, proj=True)),
            ("rag", lambda: h.encode(audio, lens, proj=True)), ("seq", lambda: [h.encode(c, proj=True) for c in clips])]
    if not a.no_whisper:
        w = native.Whisper(W_MELS, W_C, W_HEADS, a.whisper_layers, W_CTX, arch.whisper_init_state(W_MELS, W_C, a.whisper_layers, 0),
                           arch.whisper_mel_filters(W_MELS))
        legs.append(("whisper_b8", lambda: w.encode(audio)))
    for _ in range(a.warmup):
        for _, fn in legs:
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k, _ in legs}
    for _ in range(a.rounds):      # alternating: every leg sees the same clocks and the same neighbours
        for k, fn in legs:
            t[k].append(timed(fn, a.iters))
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
        print(f"B = 8 encode, profiled: {tot:.2f} ms", file=sys.stderr)
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
    if not a.no_whisper:
        fw = 8 * whisper_flop(L, a.whisper_layers)
        out.update({"whisper_layers": a.whisper_layers, "whisper_b8_ms": round(ms["whisper_b8"], 3), "whisper_b8_tflop": round(fw / 1e12, 3),
                    "whisper_b8_tflops": round(fw / ms["whisper_b8"] / 1e9, 1), "whisper_over_hubert_b8": round(ms["whisper_b8"] / ms["b8"], 3)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
