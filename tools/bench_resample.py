"""The polyphase resampler (tools.tools.Resample, lds_resample) on 30 s clips, one process, device events around whole calls after warm-up,
alternating rounds, the minimum of the rounds; one JSON line.

    python tools/bench_resample.py [--rounds 3] [--iters 5] [--no-encode]

  per (orig -> new) in 44100 -> 16000, 48000 -> 16000, 16000 -> 44100 and B in 8, 16 clips of 30 s:
    kernel      Resample.forward as a caller sees it: the Python wrapper, the output allocation and one lds_resample launch, calls back to back
    launch      the launch alone, from the library's own per-launch events (lds_prof_enable): what is left of `kernel` is host-side issue cost
    conv1d      the yardstick in the same process: torchaudio's formulation, i.e. zero padding (width, width + O), torch.nn.functional.conv1d
                with the full N x (2 width + O) bank at stride O, the transpose that interleaves the phases and the crop, all on the device
    bound       4 (B L + B M) bytes at 6.3 TB/s, what a streaming kernel reaches on this part
    max_abs_diff between the two results (fp32 rounding of two summation orders)
  encode      resample + Whisper encode of 8 clips of 30 s at 44.1 kHz against the encode alone of the 16 kHz audio (large-v3 dims, seeded weights)
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "latent-diffusion-speech_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lds import native  # noqa: E402
from tools.tools import Resample  # noqa: E402

STREAM_TBS = 6.3


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def rounds(legs, n_rounds, iters):
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in legs}
    for _ in range(n_rounds):
        for k, fn in legs.items():
            t[k].append(timed(fn, iters))
    return {k: min(v) for k, v in t.items()}


def full_bank(O, N, w=6, rolloff=0.99):
    """torchaudio's N x (2 width + O) bank (float64, rounded to fp32 once) and its width"""
    base = min(O, N) * rolloff
    width = math.ceil(w * O / base)
    j = np.arange(-width, width + O, dtype=np.int64)[None, :]
    i = np.arange(N, dtype=np.int64)[:, None]
    u = np.clip(base * (j * N - i * O) / (O * N), -w, w)
    return ((base / O) * np.sinc(u) * np.cos(np.pi * u / (2.0 * w)) ** 2).astype(np.float32), width


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--no-encode", action="store_true")
    a = ap.parse_args()
    res = {"stream_TBps": STREAM_TBS, "seconds": 30}
    g = torch.Generator(device="cuda").manual_seed(0)
    for orig, new in ((44100, 16000), (48000, 16000), (16000, 44100)):
        rs = Resample(orig, new)
        O, N, taps = rs.tables["O"], rs.tables["N"], rs.tables["taps"]
        bank, width = full_bank(O, N)
        kern = torch.from_numpy(bank).cuda()[:, None, :]
        for B in (8, 16):
            L = 30 * orig
            M = native.resample_out_length(L, O, N)
            x = torch.rand(B, L, device="cuda", generator=g) - 0.5

            def conv():
                y = torch.nn.functional.conv1d(torch.nn.functional.pad(x, (width, width + O))[:, None], kern, stride=O)
                return y.transpose(1, 2).reshape(B, -1)[:, :M].contiguous()

            ms = rounds({"kernel": lambda: rs(x), "conv1d": conv}, a.rounds, a.iters)
            bound_ms = 4.0 * (B * L + B * M) / (STREAM_TBS * 1e9)
            native.prof_enable(1)
            for _ in range(a.iters):
                rs(x)
            prof = [p for p in native.prof_summary() if p["name"] == "resample"]
            native.prof_enable(0)
            launch_ms = prof[0]["ms"] / prof[0]["count"]
            res[f"{orig}to{new}_B{B}"] = {"taps": taps, "phases": N, "full_bank_columns": bank.shape[1], "kernel_ms": round(ms["kernel"], 4), "launch_ms": round(launch_ms, 4),
                                          "conv1d_ms": round(ms["conv1d"], 4), "conv1d_over_kernel": round(ms["conv1d"] / ms["kernel"], 2),
                                          "bound_ms": round(bound_ms, 4), "kernel_over_bound": round(ms["kernel"] / bound_ms, 2), "launch_over_bound": round(launch_ms / bound_ms, 2),
                                          "max_abs_diff": float((rs(x) - conv()).abs().max())}
    if not a.no_encode:
        from lds import arch, init_weights
        hw = native.Whisper(128, 1280, 20, 32, 1500, arch.whisper_init_state(128, 1280, 32, 0), arch.whisper_mel_filters(128))
        a44 = torch.from_numpy(init_weights.uniform("bench.resample.audio", (8, 1323000), 5, -0.5, 0.5)).cuda()
        rs = Resample(44100, 16000)
        a16 = rs(a44)
        ms = rounds({"encode": lambda: hw.encode(a16), "resample_encode": lambda: hw.encode(rs(a44))}, a.rounds, 1)
        res["encode_8x30s"] = {"encode_ms": round(ms["encode"], 3), "resample_encode_ms": round(ms["resample_encode"], 3),
                               "share_on_top": round(ms["resample_encode"] / ms["encode"] - 1, 4)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
