"""The Whisper units encoder at large-v3's dims, seeded weights, one process: B = 1 and B = 8 clips of 480,000 samples, and 8 clips of
8 lengths (5 .. 30 s) as one encode_ragged call against one call per clip; warm-up, device events around whole calls, alternating
rounds; one JSON line.  `--stages` adds the per-launch split of one B = 8 encode (HIP-event profiler) on stderr, the front end's share
included.  `--layers N` runs a shallower stack (the per-layer cost is constant; the FLOP count follows).

    python tools/bench_units.py [--iters 3] [--warmup 1] [--rounds 3] [--layers 32] [--stages]
    python tools/bench_units.py --encoder wavlmbase+ | wavlmlarge | contentvec768l12 [--layers N] [--stages]
--encoder wavlmbase+ / wavlmlarge times the WavLM encoder instead (B = 8 and B = 1 clips of 30 s, seeded weights) and, in the same process and
in alternating rounds, the HuBERT-base stack (contentvec768l12: WavLM-Base+'s size without the gated position bias) on the same audio; the
difference is the price of the gate and the bias.  --encoder contentvec768l12 times that stack alone.
The per-kernel table comes from a rocprofv3 --kernel-trace --stats run of this script on its own (the front end's kernels are
logmel_power_kernel and logmel_finish_kernel)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "latent-diffusion-speech_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lds import arch, init_weights, native  # noqa: E402

PEAK_TFLOPS = 157.3            # fp32 MFMA peak of the MI355X
C, HEADS, N_MELS, N_CTX = 1280, 20, 128, 1500


def flop(n_samples, layers):
    """algorithmic FLOP of one clip: per block and frame 2 (3 + 1 + 4 + 4) C^2 plus 4 T C for attention, conv1 2 * 3 * n_mels * C per mel
    frame, conv2 2 * 3 * C^2 per frame (2.27 TFLOP at 1500 frames and 32 layers)"""
    F = n_samples // 160
    T = (F - 1) // 2 + 1
    return layers * T * (2 * 12 * C * C + 4 * T * C) + F * 2 * 3 * N_MELS * C + T * 2 * 3 * C * C


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--encoder", default="whisper_large_v3", choices=("whisper_large_v3", "contentvec768l12", "wavlmbase+", "wavlmlarge"))
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=None, help="default: the model's own depth (32 / 12 / 12 / 24)")
    ap.add_argument("--stages", action="store_true")
    return ap.parse_args(argv)


def print_stages(title, fn):
    native.prof_enable(2)
    fn()
    torch.cuda.synchronize()
    prof = native.prof_summary()
    native.prof_enable(0)
    tot = sum(r["ms"] for r in prof)
    print(f"{title}, profiled: {tot:.2f} ms", file=sys.stderr)
    for r in sorted(prof, key=lambda r: -r["ms"]):
        tf = r["flops"] / (r["ms"] * 1e-3) / 1e12 if r["flops"] else 0
        print(f"{r['name']:80s} n={r['count']:3d} {r['ms']:8.3f} ms {100 * r['ms'] / tot:5.1f}% {tf:6.1f} TF", file=sys.stderr)


def bench_conv_stack(a):
    """WavLM and / or the HuBERT-base stack on 8 clips and one clip of 30 s"""
    L = 480000
    audio = torch.from_numpy(init_weights.uniform("bench.units.audio", (8, L), 5, -0.5, 0.5)).cuda()
    legs = {}
    if a.encoder != "contentvec768l12":
        dims = arch.wavlm_dims("large" if a.encoder == "wavlmlarge" else "base+")
        dims["n_layer"] = a.layers or dims["n_layer"]
        w = native.WavLM(dims, arch.wavlm_init_state(dims, 0))
        norm = a.encoder == "wavlmlarge"
        legs["wavlm_b8"] = lambda: w.encode(audio, normalize=norm)
        legs["wavlm_b1"] = lambda: w.encode(audio[:1], normalize=norm)
    if a.encoder != "wavlmlarge":
        hd = dict(arch.HUBERT_BASE_DIMS, n_layer=a.layers or 12)
        hb = native.Hubert(hd, arch.hubert_init_state(hd, 0))
        legs["hubert_b8"] = lambda: hb.encode(audio, pad=0)
        legs["hubert_b1"] = lambda: hb.encode(audio[:1], pad=0)
    for _ in range(a.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in legs}
    for _ in range(a.rounds):      # alternating: every leg sees the same clocks and the same neighbours
        for k, fn in legs.items():
            t[k].append(timed(fn, a.iters))
    ms = {k: min(v) for k, v in t.items()}
    if a.stages:
        for k in ("wavlm_b8", "hubert_b8"):
            if k in legs:
                print_stages(k, legs[k])
    own = 24 if a.encoder == "wavlmlarge" else 12
    out = {"encoder": a.encoder, "layers": a.layers or own, "frames": arch.wavlm_frames(L), **{k + "_ms": round(v, 3) for k, v in ms.items()},
           "rounds_ms": {k: [round(x, 3) for x in v] for k, v in t.items()}}
    if "wavlm_b8" in ms and "hubert_b8" in ms:
        nl = a.layers or 12
        out["gate_bias_ms_per_layer_b8"] = round((ms["wavlm_b8"] - ms["hubert_b8"]) / nl, 4)
        out["gate_bias_ms_per_layer_b1"] = round((ms["wavlm_b1"] - ms["hubert_b1"]) / nl, 4)
        out["wavlm_over_hubert_b8"] = round(ms["wavlm_b8"] / ms["hubert_b8"], 4)
    print(json.dumps(out))


def main():
    a = parse_args()
    if a.encoder != "whisper_large_v3":
        return bench_conv_stack(a)
    a.layers = a.layers or 32
    h = native.Whisper(N_MELS, C, HEADS, a.layers, N_CTX, arch.whisper_init_state(N_MELS, C, a.layers, 0), arch.whisper_mel_filters(N_MELS))
    L = 480000
    audio = torch.from_numpy(init_weights.uniform("bench.units.audio", (8, L), 5, -0.5, 0.5)).cuda()
    lens = [80000 + (L - 80000) * i // 7 for i in range(8)]      # 5 .. 30 s
    clips = [audio[b:b + 1, :n].contiguous() for b, n in enumerate(lens)]
    b1 = lambda: h.encode(audio[:1])                        # noqa: E731
    b8 = lambda: h.encode(audio)                            # noqa: E731
    rag = lambda: h.encode(audio, lens)                     # noqa: E731
    seq = lambda: [h.encode(c) for c in clips]              # noqa: E731
    mel8 = lambda: h.logmel(audio)                          # noqa: E731
    for _ in range(a.warmup):
        b1(), b8(), rag(), seq(), mel8()
    torch.cuda.synchronize()
    t = {k: [] for k in ("b1", "b8", "rag", "seq", "mel8")}
    for _ in range(a.rounds):      # alternating: every leg sees the same clocks and the same neighbours
        for k, fn in (("b1", b1), ("b8", b8), ("rag", rag), ("seq", seq), ("mel8", mel8)):
            t[k].append(timed(fn, a.iters))
    ms = {k: min(v) for k, v in t.items()}
    f1, f8, fr = flop(L, a.layers), 8 * flop(L, a.layers), sum(flop(n, a.layers) for n in lens)
    if a.stages:
        print_stages("B = 8 encode", b8)
    print(json.dumps({
        "layers": a.layers, "b1_ms": round(ms["b1"], 3), "b8_ms": round(ms["b8"], 3), "ragged8_ms": round(ms["rag"], 3), "per_clip8_ms": round(ms["seq"], 3),
        "logmel8_ms": round(ms["mel8"], 3), "front_end_share_b8": round(ms["mel8"] / ms["b8"], 4),
        "b1_tflop": round(f1 / 1e12, 3), "b8_tflop": round(f8 / 1e12, 3), "ragged8_tflop": round(fr / 1e12, 3),
        "b1_tflops": round(f1 / ms["b1"] / 1e9, 1), "b8_tflops": round(f8 / ms["b8"] / 1e9, 1), "ragged8_tflops": round(fr / ms["rag"] / 1e9, 1),
        "per_clip8_tflops": round(fr / ms["seq"] / 1e9, 1), "b8_frac_peak": round(f8 / ms["b8"] / 1e9 / PEAK_TFLOPS, 3),
        "per_clip_over_ragged": round(ms["seq"] / ms["rag"], 3), "rounds_ms": {k: [round(x, 3) for x in v] for k, v in t.items()},
        "ragged_lengths": lens}))


if __name__ == "__main__":
    main()
