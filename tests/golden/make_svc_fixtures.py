"""Generate the long-audio fixtures by running the reference's own tools/slicer.py and tools/tools.py.

Runs ONLY in the build container (needs the reference checkout); the GPU box never sees the reference.  Writes (default: next to this
script, `--out DIR` elsewhere):

  svc.npz             clip (the fixture clip of tests/svc_numpy.py make_clip at 16 kHz, fp32), rms_<win>_<hop> (the frame RMS the reference's
                      Slicer saw at that window and hop, float64 [n]: rms_1280_320 and rms_640_160), vol_<i> (Volume_Extractor.extract of the clip at hop HOPS[i], float64), mask_in / mask_<j>
                      (a 60-frame volume and get_mask_from_volume of it at THRESHOLDS[j] dB, block_size 512, fp32 [1, n * 512]),
                      up_in / up_out (upsample of a [1, 7, 2] signal by 5), xf_<k>_a / _b / _out (cross_fade cases, idx in the manifest)
  manifest_svc.json   for every Slicer parameter set the chunk dict that Slicer.slice returned; for every (hop_size, db_thresh, min_len)
                      the (start_frame, begin, end) of the segments that split returned (every segment checked to be audio[begin:end]);
                      the hops, thresholds and cross-fade indices

librosa, torchaudio, fairseq and transformers are absent here: import-only placeholders stand in, and the two librosa functions the slicer
calls, feature.rms and to_mono, are the float64 restatements of tests/svc_numpy.py (librosa >= 0.10's zero padding).  The array the
slicer receives from feature.rms is a watched ndarray: every arg-min it takes asserts that the runner-up is at least MARGIN (relative)
above the minimum, and every frame's RMS (and every volume against every mask threshold) is asserted to be at least MARGIN away from
the threshold -- five times the fp32 bound of the device's RMS, so that the device's values cannot change a recorded decision.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_svc_fixtures.py [--out DIR] [--ref DIR]
    python tests/golden/make_svc_fixtures.py --verify      # regenerate into a temporary directory, compare bit for bit
"""
import argparse
import importlib.machinery
import importlib.util
import json
import os
import subprocess
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PKG = os.path.join(ROOT, "latent-diffusion-speech_amd")
REF = "/root/reference"
FILES = ("manifest_svc.json", "svc.npz")
MARGIN = 1e-3
SR = 16000
# Slicer(sr, threshold, min_length, min_interval, hop_size, max_sil_kept): the three max_sil_kept branches, two clip lengths, two thresholds
SLICERS = [dict(threshold=-40., min_length=1000, min_interval=300, hop_size=20, max_sil_kept=5000),
           dict(threshold=-40., min_length=1000, min_interval=300, hop_size=20, max_sil_kept=500),
           dict(threshold=-40., min_length=500, min_interval=300, hop_size=20, max_sil_kept=200),
           dict(threshold=-40., min_length=5000, min_interval=300, hop_size=20, max_sil_kept=5000),
           dict(threshold=-30., min_length=500, min_interval=300, hop_size=20, max_sil_kept=500),
           dict(threshold=-40., min_length=500, min_interval=300, hop_size=10, max_sil_kept=300)]
HOPS = [320.0, 512 * 16000 / 44100, 512.0, 3.5]
SPLITS = [(HOPS[0], -40, 1000), (HOPS[1], -40, 1000), (HOPS[0], -40, 500), (HOPS[1], -40, 500), (HOPS[1], -40, 5000), (HOPS[1], -30, 500)]
THRESHOLDS = [-60.0, -45.0, -20.0]
CROSS_FADES = [(1000, 800, 999), (1000, 800, 488), (300, 300, 0), (50, 70, 50)]      # (len a, len b, idx): F = 1, 512, the whole of a, 0
sys.dont_write_bytecode = True


def _load_by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _placeholder(name, **attrs):
    m = types.ModuleType(name)
    m.__spec__ = importlib.machinery.ModuleSpec(name, None)
    for k, v in attrs.items():
        setattr(m, k, v)
    return sys.modules.setdefault(name, m)


class Watched(np.ndarray):
    """the RMS as the slicer holds it: an arg-min without a clear winner is an error of the fixture, not a recorded result"""

    def argmin(self, *a, **k):
        v = np.sort(np.asarray(self).reshape(-1))
        assert len(v) < 2 or v[1] - v[0] >= MARGIN * v[0], f"arg-min runner-up {v[1]} within {MARGIN} of the minimum {v[0]}"
        return np.asarray(self).argmin(*a, **k)


def verify(ref):
    with tempfile.TemporaryDirectory() as out_dir:
        env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
        env.pop("PYTHONPATH", None)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--out", out_dir, "--ref", ref], env=env, cwd=out_dir, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            print(r.stdout[-4000:])
            return 1
        bad = []
        if json.load(open(os.path.join(HERE, FILES[0]))) != json.load(open(os.path.join(out_dir, FILES[0]))):
            bad.append(FILES[0])
        za, zb = np.load(os.path.join(HERE, FILES[1])), np.load(os.path.join(out_dir, FILES[1]))
        if sorted(za.files) != sorted(zb.files):
            bad.append(FILES[1])
        else:
            bad += [f"{FILES[1]}:{k}" for k in za.files if za[k].dtype != zb[k].dtype or za[k].shape != zb[k].shape or za[k].tobytes() != zb[k].tobytes()]
        print("svc fixtures", "differ: " + ", ".join(bad) if bad else "reproduce bit for bit")
        return 1 if bad else 0


def main(out, ref):
    sn = _load_by_path("_amd_svc_numpy", os.path.join(ROOT, "tests", "svc_numpy.py"))
    sys.path[:] = [p for p in sys.path if os.path.realpath(p or ".") not in (os.path.realpath(PKG), os.path.realpath(ROOT), os.path.realpath(HERE))]
    sys.path.insert(0, ref)
    import torch
    torch.set_grad_enabled(False)
    seen = {}

    def rms(y, frame_length, hop_length):
        r = sn.frame_rms(y, frame_length, hop_length)
        seen["rms"] = r
        return r[None, :].view(Watched)
    _placeholder("librosa", feature=types.SimpleNamespace(rms=rms), to_mono=sn.to_mono)
    _placeholder("fairseq", checkpoint_utils=None)
    _placeholder("transformers", AutoFeatureExtractor=object, Wav2Vec2BertModel=object)
    _tat = _placeholder("torchaudio.transforms", Resample=object)
    _placeholder("torchaudio", transforms=_tat)
    from tools import slicer as ref_slicer, tools as ref_tools
    for m in (ref_slicer, ref_tools):
        f = os.path.realpath(m.__file__)
        assert f.startswith(os.path.realpath(ref) + os.sep), f"{m} was imported from {f}, not from the reference"

    clip = sn.make_clip(SR)
    arrays, manifest = {"clip": clip}, {"sr": SR, "slicers": [], "splits": [], "hops": HOPS, "thresholds": THRESHOLDS, "cross_fades": []}

    def clear_of(values, thr, what):
        gap = np.abs(np.asarray(values, dtype=np.float64) - thr).min() / thr
        assert gap >= MARGIN, f"{what}: a value within {gap:.2e} (relative) of the threshold {thr}"

    # ---- Slicer.slice ----
    for i, kw in enumerate(SLICERS):
        s = ref_slicer.Slicer(sr=SR, **kw)
        chunks = s.slice(clip)
        clear_of(seen["rms"], s.threshold, f"slicer {i}")
        arrays[f"rms_{s.win_size}_{s.hop_size}"] = seen["rms"]
        manifest["slicers"].append({"args": kw, "rms": f"rms_{s.win_size}_{s.hop_size}", "chunks": chunks})
        print(f"slicer {i}: {len(chunks)} chunks", [c["split_time"] for c in chunks.values()])

    # ---- split ----
    for hop, db, min_len in SPLITS:
        segs = ref_slicer.split(clip, SR, hop, db_thresh=db, min_len=min_len)
        rows = []
        for start_frame, seg in segs:
            begin = int(start_frame * hop)
            assert np.array_equal(seg, clip[begin: begin + len(seg)])
            rows.append([int(start_frame), begin, begin + len(seg)])
        manifest["splits"].append({"hop_size": hop, "db_thresh": db, "min_len": min_len, "segments": rows})
        joins = [int(rows[k + 1][0]) - (rows[k][0] + int((rows[k][2] - rows[k][1]) // hop) + 1) for k in range(len(rows) - 1)]
        print(f"split hop {hop:.2f} db {db} min_len {min_len}: {len(rows)} segments, frames between neighbours {joins}")

    # ---- volume, mask, upsample ----
    for i, hop in enumerate(HOPS):
        ve = ref_tools.Volume_Extractor(hop_size=hop)
        arrays[f"vol_{i}"] = ve.extract(clip.astype(np.float64))
    ve = ref_tools.Volume_Extractor(hop_size=512, block_size=512, model_sampling_rate=44100)
    vol = ve.extract(clip[:11000].astype(np.float64), SR)
    assert len(vol) <= 64
    arrays["mask_in"] = vol
    for j, db in enumerate(THRESHOLDS):
        clear_of(vol, 10 ** (db / 20), f"mask threshold {db}")
        arrays[f"mask_{j}"] = ve.get_mask_from_volume(vol, threhold=db).numpy()
    up_in = (np.arange(14, dtype=np.float32).reshape(1, 7, 2) % 5) * 0.25
    arrays["up_in"], arrays["up_out"] = up_in, ref_tools.upsample(torch.from_numpy(up_in), 5).numpy()

    # ---- cross_fade ----
    for k, (la, lb, idx) in enumerate(CROSS_FADES):
        a, b = clip[10000: 10000 + la].astype(np.float64), clip[40000: 40000 + lb].astype(np.float64)
        arrays[f"xf_{k}_a"], arrays[f"xf_{k}_b"], arrays[f"xf_{k}_out"] = a, b, ref_tools.cross_fade(a, b, idx)
        manifest["cross_fades"].append(idx)

    np.savez_compressed(os.path.join(out, FILES[1]), **arrays)
    json.dump(manifest, open(os.path.join(out, FILES[0]), "w"), indent=0)
    print("wrote", ", ".join(FILES), "to", out, f"({os.path.getsize(os.path.join(out, FILES[1]))} bytes)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    ap.add_argument("--ref", default=REF)
    ap.add_argument("--verify", action="store_true")
    a = ap.parse_args()
    sys.exit(verify(a.ref) if a.verify else main(a.out, a.ref))
