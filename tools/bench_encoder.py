"""The VAE encoder against the decoder, same process, seeded weights: Hifi_VAEGAN.extract of 16 x 262,144 samples and Vocoder.infer of
16 x 512 frames, alternating, timed with device events; the B = 1 x 512-frame encoder latency; one JSON line.  `--stages` adds the
per-stage split of one encode (HIP-event profiler at shape detail) on stderr.  `--ragged` times 16 clips of 16 lengths instead
(272 .. 512 frames, n * 512 - 37 samples each): (a) one extract_ragged call, (b) the same clips as one padded extract (the reference's
batch behaviour), (c) one extract per clip in turn; one JSON line.

    python tools/bench_encoder.py [--iters 10] [--warmup 3] [--stages] [--ragged]
The per-kernel table comes from a rocprofv3 --kernel-trace --stats run of this script on its own."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "latent-diffusion-speech_amd"))
import torch  # noqa: E402

from diffusion.vocoder import Vocoder  # noqa: E402
from encoder.hifi_vaegan.hifi_vaegan import Hifi_VAEGAN  # noqa: E402
from lds import arch, init_weights, native  # noqa: E402

PEAK_TFLOPS = 157.3            # fp32 MFMA peak of the MI355X
ENC_TFLOP, DEC_TFLOP = 5.585, 5.310      # 16 x 512 frames, from the layer shapes
B, T, HOP = 16, 512, 512


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
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--stages", action="store_true")
    ap.add_argument("--ragged", action="store_true", help="16 clips of 16 lengths: ragged vs padded vs one call per clip")
    a = ap.parse_args()
    h = arch.SYNTHETIC_VOCODER_H
    vae = Hifi_VAEGAN(None, device="cuda", h=h, state=init_weights.init_state(arch.generator_param_shapes(h), 0),
                      encoder_state=init_weights.init_state(arch.encoder_param_shapes(h), 0))
    voc = Vocoder.__new__(Vocoder)
    voc.vocoder = vae
    audio = torch.from_numpy(init_weights.uniform("bench.enc.audio", (B, T * HOP), 5, -0.5, 0.5)).cuda()
    if a.ragged:
        return ragged(vae, audio, a)
    mel = torch.from_numpy(init_weights.uniform("voc.mel", (B, T, 80), 5, -1, 1)).cuda()
    enc = lambda: vae.extract(audio)      # noqa: E731
    dec = lambda: voc.infer(mel)          # noqa: E731
    enc1 = lambda: vae.extract(audio[:1])  # noqa: E731
    for _ in range(a.warmup):
        enc(), dec(), enc1()
    torch.cuda.synchronize()
    te, td, t1 = [], [], []
    for _ in range(a.rounds):      # alternating: both legs see the same clocks and the same neighbours
        te.append(timed(enc, a.iters))
        td.append(timed(dec, a.iters))
        t1.append(timed(enc1, a.iters))
    ms_e, ms_d, ms_1 = min(te), min(td), min(t1)
    if a.stages:
        native.prof_enable(2)
        enc()
        torch.cuda.synchronize()
        prof = native.prof_summary()
        native.prof_enable(0)
        tot = sum(r["ms"] for r in prof)
        print(f"encode, profiled: {tot:.2f} ms", file=sys.stderr)
        for r in sorted(prof, key=lambda r: -r["ms"]):
            tf = r["flops"] / (r["ms"] * 1e-3) / 1e12 if r["flops"] else 0
            print(f"{r['name']:80s} n={r['count']:3d} {r['ms']:7.2f} ms {100 * r['ms'] / tot:5.1f}% {tf:6.1f} TF", file=sys.stderr)
    print(json.dumps({
        "encoder_ms": round(ms_e, 3), "decoder_ms": round(ms_d, 3), "ratio": round(ms_e / ms_d, 3),
        "encoder_tflop": ENC_TFLOP, "decoder_tflop": DEC_TFLOP,
        "encoder_tflops": round(ENC_TFLOP / ms_e * 1e3, 1), "decoder_tflops": round(DEC_TFLOP / ms_d * 1e3, 1),
        "encoder_frac_peak": round(ENC_TFLOP / ms_e * 1e3 / PEAK_TFLOPS, 3), "decoder_frac_peak": round(DEC_TFLOP / ms_d * 1e3 / PEAK_TFLOPS, 3),
        "encoder_b1_ms": round(ms_1, 3), "encoder_ms_rounds": [round(x, 3) for x in te], "decoder_ms_rounds": [round(x, 3) for x in td],
        "shape": f"B={B} x {T} frames ({T * HOP} samples)"}))


def ragged(vae, audio, a):
    lens = [(272 + 16 * i) * HOP - 37 for i in range(B)]
    audio = audio.clone()
    for b, n in enumerate(lens):
        audio[b, n:] = 0.0      # the padded batch (b) sees zeros there, as the reference's batch loader pads
    clips = [audio[b:b + 1, :n].contiguous() for b, n in enumerate(lens)]
    rag = lambda: vae.extract_ragged(audio, lens)                 # noqa: E731
    pad = lambda: vae.extract(audio)                              # noqa: E731
    seq = lambda: [vae.extract(c) for c in clips]                 # noqa: E731
    for _ in range(a.warmup):
        rag(), pad(), seq()
    torch.cuda.synchronize()
    tr, tp, ts = [], [], []
    for _ in range(a.rounds):
        tr.append(timed(rag, a.iters))
        tp.append(timed(pad, a.iters))
        ts.append(timed(seq, max(1, a.iters // 4)))
    ms_r, ms_p, ms_s = min(tr), min(tp), min(ts)
    print(json.dumps({
        "ragged_ms": round(ms_r, 3), "padded_ms": round(ms_p, 3), "per_clip_ms": round(ms_s, 3),
        "ragged_over_padded": round(ms_r / ms_p, 3), "per_clip_over_ragged": round(ms_s / ms_r, 3),
        "ragged_ms_rounds": [round(x, 3) for x in tr], "padded_ms_rounds": [round(x, 3) for x in tp], "per_clip_ms_rounds": [round(x, 3) for x in ts],
        "frames": sum(-(-n // HOP) for n in lens), "shape": f"{B} clips of {min(lens)} .. {max(lens)} samples in a {T}-frame buffer"}))


if __name__ == "__main__":
    main()
