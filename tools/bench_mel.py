"""The vocoder's log-mel analysis against the decoder, same process, seeded weights: Hifi_VAEGAN.get_mel of 16 x 262,144 samples and
Vocoder.infer of 16 x 512 frames on the same batch, alternating, timed with device events; get_mel of one clip; one JSON line with the
times and the f64 matrix rate the framed DFT reaches (4 * n_fft * bins flop per frame: the cos and the sin product).

    python tools/bench_mel.py [--iters 10] [--warmup 3] [--rounds 3] [--keyshift 0]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "latent-diffusion-speech_amd"))
import torch  # noqa: E402

from diffusion.vocoder import Vocoder  # noqa: E402
from encoder.hifi_vaegan.hifi_vaegan import Hifi_VAEGAN  # noqa: E402
from lds import arch, init_weights, stftmel  # noqa: E402

PEAK_F64_TFLOPS = 78.6         # f64 matrix peak of the MI355X
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
    ap.add_argument("--keyshift", type=float, default=0)
    a = ap.parse_args()
    h = arch.SYNTHETIC_VOCODER_H
    vae = Hifi_VAEGAN(None, device="cuda", h=h, state=init_weights.init_state(arch.generator_param_shapes(h), 0))
    voc = Vocoder.__new__(Vocoder)
    voc.vocoder = vae
    z = torch.from_numpy(init_weights.uniform("voc.mel", (B, T, h["inter_channels"]), 5, -1, 1)).cuda()
    wav = voc.infer(z)[:, 0].contiguous()      # [B, T * HOP]: the analysis runs on what the decoder made
    ks = int(a.keyshift) if a.keyshift == int(a.keyshift) else a.keyshift
    mel = lambda: vae.get_mel(wav, keyshift=ks)            # noqa: E731
    dec = lambda: voc.infer(z)                             # noqa: E731
    mel1 = lambda: vae.get_mel(wav[:1], keyshift=ks)       # noqa: E731
    for _ in range(a.warmup):
        mel(), dec(), mel1()
    torch.cuda.synchronize()
    tm, td, t1 = [], [], []
    for _ in range(a.rounds):      # alternating: both legs see the same clocks and the same neighbours
        tm.append(timed(mel, a.iters))
        td.append(timed(dec, a.iters))
        t1.append(timed(mel1, a.iters))
    ms_m, ms_d, ms_1 = min(tm), min(td), min(t1)
    n_fft_new, win_new, hop_new = stftmel.geometry(vae.stft.n_fft, vae.stft.win_size, vae.stft.hop_length, ks, 1)
    bins = min(n_fft_new // 2 + 1, vae.stft.n_fft // 2 + 1)
    F = stftmel.frames(T * HOP, n_fft_new, win_new, hop_new)
    tflop = 4.0 * n_fft_new * bins * F * B / 1e12
    print(json.dumps({
        "mel_ms": round(ms_m, 3), "decoder_ms": round(ms_d, 3), "ratio": round(ms_m / ms_d, 3), "mel_b1_ms": round(ms_1, 3),
        "dft_tflop": round(tflop, 4), "f64_tflops": round(tflop / ms_m * 1e3, 2), "f64_frac_peak": round(tflop / ms_m * 1e3 / PEAK_F64_TFLOPS, 3),
        "f64_tflops_b1": round(tflop / B / ms_1 * 1e3, 2),
        "mel_ms_rounds": [round(x, 3) for x in tm], "decoder_ms_rounds": [round(x, 3) for x in td], "mel_b1_ms_rounds": [round(x, 3) for x in t1],
        "keyshift": ks, "n_fft_new": n_fft_new, "frames": F, "shape": f"B={B} x {T * HOP} samples ({F} frames each)"}))


if __name__ == "__main__":
    main()
