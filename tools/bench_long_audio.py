"""DiffusionSVC.infer_from_long_audio on a synthetic recording of about five minutes (infer_svc.synthetic_recording: a few dozen segments of
4 .. 12 s after the slicer), seeded weights at product size (Unit2Mel 1280 -> 80, the seeded vocoder, a Whisper encoder of large-v3's width
with `--layers` blocks), one process: batch_size 1 -- the reference's loop shape, one segment per encoder / sampler / vocoder call --
against batch_size 16.  Warm-up, then `--rounds` alternating rounds, wall time around whole calls with a device synchronisation either side
(the method's host work -- the RMS copy, the slicer's decisions, the packing -- is part of what a caller waits for); one JSON line with the
median and the run-to-run spread (min .. max) of each.

    python tools/bench_long_audio.py [--seconds 300] [--rounds 3] [--warmup 1] [--layers 4] [--speedup 10]
    python tools/bench_long_audio.py --share      # the new kernels' share: runs itself once under rocprofv3 --kernel-trace --stats
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "latent-diffusion-speech_amd"))

NEW_KERNELS = ("frame_rms_kernel", "volume_kernel", "volume_mask_kernel", "resample_frames_ragged_kernel", "overlap_assemble_kernel")


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=300.0)
    ap.add_argument("--sample_rate", type=int, default=44100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--speedup", type=int, default=10)
    ap.add_argument("--batch_sizes", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--share", action="store_true")
    ap.add_argument("--share_timeout", type=float, default=600.0, help="seconds the profiled child of --share may take")
    return ap.parse_args()


def share(a):
    """one run of this script (one round, no warm-up, batch_size 16) under the profiler; the share of NEW_KERNELS in the summed kernel time"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "ks", "--", sys.executable, os.path.abspath(__file__),
               "--seconds", str(a.seconds), "--sample_rate", str(a.sample_rate), "--rounds", "1", "--warmup", "0", "--layers", str(a.layers),
               "--speedup", str(a.speedup), "--batch_sizes", "16"]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.share_timeout)
        if r.returncode != 0:
            print(r.stdout[-3000:])
            return 1
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            print("no kernel_stats.csv under", d, os.listdir(d))
            return 1
        rows = list(csv.DictReader(open(files[0])))
    print(json.dumps(share_of(rows)))
    return 0


def share_of(rows):
    """rows of a rocprofv3 kernel_stats.csv (Name, Calls, TotalDurationNs, ...) -> the JSON record: the summed kernel time, NEW_KERNELS' part
    of it and every new kernel's calls and time"""
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    new = {k: (0, 0.0) for k in NEW_KERNELS}
    for r in rows:
        for k in NEW_KERNELS:
            if "lds::" + k + "(" in r["Name"]:
                new[k] = (new[k][0] + int(r["Calls"]), new[k][1] + float(r["TotalDurationNs"]))
    part = sum(v[1] for v in new.values())
    return {"metric": "long_audio_new_kernel_share", "kernel_time_ms": total / 1e6, "new_kernels_ms": part / 1e6, "share": part / total,
            "per_kernel": {k: {"calls": v[0], "us": v[1] / 1e3} for k, v in new.items()}}


def main():
    a = parse()
    if a.share:
        return share(a)
    import torch
    import infer_svc
    from tools.slicer import split_ranges
    svc = infer_svc.synthetic_svc("cuda", width=1280, layers=a.layers)
    rec = torch.from_numpy(infer_svc.synthetic_recording(a.seconds, a.sample_rate)).cuda()
    ranges = split_ranges(rec, a.sample_rate, 512 * a.sample_rate / 44100)
    secs = [(e - b) / a.sample_rate for _, b, e in ranges]

    def run(bs):
        torch.manual_seed(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        wav, _ = svc.infer_from_long_audio(rec, sr=a.sample_rate, infer_speedup=a.speedup, batch_size=bs)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, wav
    times = {bs: [] for bs in a.batch_sizes}
    for _ in range(a.warmup):
        for bs in a.batch_sizes:
            run(bs)
    n_out = 0
    for _ in range(a.rounds):
        for bs in a.batch_sizes:      # alternating: a drift of the clocks lands on both
            t, wav = run(bs)
            times[bs].append(t)
            n_out = wav.numel()
    out = {"metric": "long_audio_seconds", "recording_s": a.seconds, "sample_rate": a.sample_rate, "segments": len(ranges),
           "segment_s": [round(min(secs), 2), round(statistics.median(secs), 2), round(max(secs), 2)], "out_samples": n_out,
           "sampler_steps": 1000 // a.speedup, "whisper_layers": a.layers, "rounds": a.rounds}
    for bs, ts in times.items():
        out[f"batch_size_{bs}"] = {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts)}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
