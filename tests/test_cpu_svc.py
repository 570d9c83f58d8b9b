"""Host side of the long-audio path (no GPU): the slicer's decisions and the segment ranges against what the reference's own Slicer / split
recorded (tests/golden/svc.npz + manifest_svc.json, made by tests/golden/make_svc_fixtures.py), the float64 restatements of
tests/svc_numpy.py against the reference's recorded volume, mask, upsample and cross-fades, and the validation that runs before any device
call."""
import json
import os

import numpy as np
import pytest

import svc_numpy as SN
from conftest import GOLDEN


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "svc.npz"))), json.load(open(os.path.join(GOLDEN, "manifest_svc.json")))


def test_fixture_clip_is_the_generated_one(fx):
    z, man = fx
    assert man["sr"] == 16000 and z["clip"].dtype == np.float32 and z["clip"].shape == (85600,)
    assert np.abs(z["clip"].astype(np.float64) - SN.make_clip(16000, np.float64)).max() < 1e-7      # (sin may differ in its last bit elsewhere)


def test_slice_from_rms_reproduces_every_recorded_chunk_dict(fx):
    from tools.slicer import Slicer
    z, man = fx
    assert len(man["slicers"]) >= 6
    seen = set()
    for rec in man["slicers"]:
        s = Slicer(sr=man["sr"], **rec["args"])
        rms = z[rec["rms"]]
        assert rec["rms"] == f"rms_{s.win_size}_{s.hop_size}" and len(rms) == SN.frame_rms_length(85600, s.win_size, s.hop_size)
        assert s.slice_from_rms(rms, 85600) == rec["chunks"], rec["args"]
        seen.add(len(rec["chunks"]))
        # the recorded RMS is the restatement's (the recipe hands it to the reference's Slicer as librosa's)
        assert np.array_equal(SN.frame_rms(z["clip"], s.win_size, s.hop_size), rms)
    assert {2, 6, 7} <= seen
    assert Slicer(16000).slice_from_rms(None, 250) == {"0": {"slice": False, "split_time": "0,250"}}      # the early exit: 250 samples <= 250 frames


def test_split_ranges_reproduce_every_recorded_segment_list(fx):
    from tools.slicer import Slicer, split_ranges
    z, man = fx
    joins = set()
    for rec in man["splits"]:
        s = Slicer(sr=man["sr"], threshold=rec["db_thresh"], min_length=rec["min_len"])
        got = split_ranges(z["clip"], man["sr"], rec["hop_size"], rec["db_thresh"], rec["min_len"], rms_list=z[f"rms_{s.win_size}_{s.hop_size}"])
        assert [list(g) for g in got] == rec["segments"], rec
        hop = rec["hop_size"]
        for (f0, b0, e0), (f1, _, _) in zip(got, got[1:]):
            joins.add((hop == 320.0, f1 - (f0 + int((e0 - b0) // hop) + 1)))
    assert {(True, -1), (False, -1), (False, 0)} <= joins      # one-frame overlaps at both hops, exact abutment at the fractional one


def test_restatements_reproduce_the_recorded_volume_mask_and_cross_fades(fx):
    z, man = fx
    for i, hop in enumerate(man["hops"]):
        got = SN.volume(z["clip"], hop)
        assert got.shape == z[f"vol_{i}"].shape and np.abs(got - z[f"vol_{i}"]).max() <= 1e-15 * max(1.0, z[f"vol_{i}"].max())
    vol = z["mask_in"]
    assert len(vol) <= 64
    states = set()
    for j, db in enumerate(man["thresholds"]):
        ref = z[f"mask_{j}"]
        got = SN.mask(vol, 10 ** (db / 20), 512)
        assert ref.shape == (1, len(vol) * 512)
        # the reference interpolates at an fp32 source position: one spacing at position n, 64 * 2^-23 < 1e-5
        assert np.abs(got - ref[0]).max() < 1e-5
        states.add((bool(got.min() == 0), bool(got.max() == 1)))
    assert (True, True) in states      # a threshold that splits the volumes
    up = z["up_in"].astype(np.float64)
    n, f = up.shape[1], 5
    j = np.arange(n * f)
    want = up[:, j // f] * (1 - (j % f) / f)[None, :, None] + up[:, np.minimum(j // f + 1, n - 1)] * ((j % f) / f)[None, :, None]
    assert np.abs(want - z["up_out"]).max() < 1e-6
    for k, idx in enumerate(man["cross_fades"]):
        a, b, ref = z[f"xf_{k}_a"], z[f"xf_{k}_b"], z[f"xf_{k}_out"]
        got = SN.assemble([a, b], [0, idx])
        assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-16


def test_slicer_conditions_and_unbuilt_loaders():
    import torch
    from tools import slicer
    with pytest.raises(ValueError, match="min_length >= min_interval >= hop_size"):
        slicer.Slicer(16000, min_length=200, min_interval=300)
    with pytest.raises(ValueError, match="min_length >= min_interval >= hop_size"):
        slicer.Slicer(16000, min_interval=10, hop_size=20)
    with pytest.raises(ValueError, match="max_sil_kept >= hop_size"):
        slicer.Slicer(16000, max_sil_kept=10)
    s = slicer.Slicer(44100)
    assert (s.hop_size, s.win_size, s.min_length, s.min_interval, s.max_sil_kept) == (882, 3528, 250, 15, 250) and abs(s.threshold - 0.01) < 1e-12
    with pytest.raises(ValueError, match="mono"):
        s.slice(np.zeros((2, 100000), dtype=np.float32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.slice(torch.zeros(100000))
    with pytest.raises(NotImplementedError):
        slicer.cut("a.wav")
    with pytest.raises(NotImplementedError):
        slicer.chunks2audio("a.wav", {})


def test_assemble_preconditions_are_checked_on_the_host():
    """lds_overlap_assemble validates the host copy of the table before it touches a device pointer: called here without a GPU, null device
    pointers; a table that passes every precondition gets as far as the null-pointer check"""
    from lds import native
    L = native.lib()

    def refuse(off, start, ln, segs_len, mask_len, N=None):
        tab = native.overlap_table(off, start, ln)
        N = int(tab[1, -1] + tab[2, -1]) if N is None else N
        fake_mask = 1 if mask_len is not None else None      # (never dereferenced: the length check comes first)
        assert L.lds_overlap_assemble(None, segs_len, tab.ctypes.data, None, tab.shape[1], fake_mask, mask_len or 0, None, N, None) == -1
        return L.lds_last_error().decode()
    assert "null pointer" in refuse([0, 10, 30], [0, 9, 40], [10, 20, 5], 35, 45)
    cases = {
        "segment 1: start 5 below": ([0, 10], [6, 5], [10, 10], 20, None),
        "segment 1: the overlap of 8 samples": ([0, 10], [0, 2], [10, 3], 13, None),
        "segment 2: start 8 inside segment 0": ([0, 10, 30], [0, 7, 8], [10, 20, 30], 60, None),
        "segment 1: offset 10": ([0, 10], [0, 10], [10, 11], 20, None),
        "the mask holds 19 samples": ([0, 10], [0, 10], [10, 10], 20, 19),
    }
    for msg, args in cases.items():
        assert msg in refuse(*args), (msg, refuse(*args))
    assert "N 30, must be 29" in refuse([0, 10], [0, 9], [10, 20], 30, None, N=30)
    with pytest.raises(ValueError, match="no segment"):
        native.overlap_table([], [], [])


def test_library_refuses_bad_arguments_before_any_device_call():
    """the C entries validate on the host: callable without a GPU with null device pointers"""
    import ctypes as C
    from lds import native
    L = native.lib()

    def err(rc, text):
        assert rc == -1 and text in L.lds_last_error().decode(), (rc, L.lds_last_error())
    err(L.lds_frame_rms(None, None, 1000, 1280, 320, 0, 5, None), "n 5, must be 4")
    err(L.lds_frame_rms(None, None, 1000, 1280, 0, 0, 4, None), "hop_length 0")
    err(L.lds_frame_rms(None, None, 1000, 1280, 320, 2, 4, None), "pad_mode 2")
    err(L.lds_frame_rms(None, None, 1000, 1280, 320, 0, 4, None), "null pointer")
    hop = C.c_double(185.75963718820861)
    err(L.lds_volume_extract(None, None, 85600, C.addressof(hop), 460, None), "n 460, must be 461")
    err(L.lds_volume_extract(None, None, 93, C.addressof(hop), 1, None), "must exceed")
    half = C.c_double(0.5)
    err(L.lds_volume_extract(None, None, 85600, C.addressof(half), 1, None), "hop 0.5")
    err(L.lds_volume_mask(None, None, 0, 512, 0.001, None), "n 0")
    err(L.lds_volume_mask(None, None, 10, 0, 0.001, None), "factor 0")
    tin, tout = (C.c_int32 * 2)(5, 9), (C.c_int32 * 2)(7, 3)
    err(L.lds_resample_frames_ragged(None, tin, tout, None, 2, 8, 7, 4, None), "tin[1] = 9")
    err(L.lds_resample_frames_ragged(None, tin, tout, None, 65, 9, 7, 4, None), "B 65")
    tab = native.overlap_table([0, 10, 30], [0, 7, 8], [10, 20, 30])
    err(L.lds_overlap_assemble(None, 60, tab.ctypes.data, None, 3, None, 0, None, 38, None), "segment 2")
    tab = native.overlap_table([0, 10], [0, 9], [10, 20])
    err(L.lds_overlap_assemble(None, 30, tab.ctypes.data, None, 2, None, 0, None, 30, None), "N 30, must be 29")


class _Args(dict):
    pass


def test_infer_from_long_audio_host_validation():
    import torch
    from tools.infer_tools import DiffusionSVC
    svc = DiffusionSVC(device="cpu")
    audio = np.zeros(16000, dtype=np.float32)
    with pytest.raises(NotImplementedError, match="key"):
        svc.infer_from_long_audio(audio, sr=16000, key=3)
    for bs in (0, 65):
        with pytest.raises(ValueError, match="batch_size"):
            svc.infer_from_long_audio(audio, sr=16000, batch_size=bs)
    with pytest.raises(NotImplementedError, match="units encoder"):
        svc.infer_from_long_audio(audio, sr=16000)
    # the plan: frame counts, stable sort by length, chunks; a segment over the window is named
    from encoder.whisper.model import ModelDimensions
    from lds import arch
    from tools.tools import Units_Encoder, Volume_Extractor, WhisperLargeV3
    dims = ModelDimensions(**dict(arch.WHISPER_LARGE_V3_DIMS, n_audio_state=64, n_audio_head=1, n_audio_layer=1))
    svc.units_encoder = Units_Encoder("whisper_large_v3", device="cpu", model=WhisperLargeV3.synthetic(dims, device="cpu"), resample=True)
    svc.args = {"data": {"block_size": 512, "sampling_rate": 44100}}
    ranges = [(0, 0, 30000), (170, 31000, 31500), (180, 33000, 63000), (400, 70000, 78000)]
    plan = svc._plan_long_audio(44100, ranges, batch_size=3)
    assert plan["hop_size"] == 512.0 and plan["n_frames"] == [59, 1, 59, 16]
    assert plan["chunks"] == [[1, 3, 0], [2]]
    with pytest.raises(ValueError, match="segment 1 .*exceeds the units encoder's window"):
        svc._plan_long_audio(44100, [(0, 0, 1000), (2, 1024, 1024 + 1324000)], batch_size=3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        svc.infer_from_long_audio(torch.zeros(16000), sr=16000)
    ve = Volume_Extractor(hop_size=512, block_size=512, model_sampling_rate=44100)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ve.extract(torch.zeros(16000), 16000)
    assert ve.hop_size == 512 * 16000 / 44100


def test_bench_long_audio_reads_a_kernel_stats_table(tmp_path):
    """the share mode's reading of rocprofv3's kernel_stats.csv, on a committed table of that format with the new kernels' rows added"""
    import csv
    import importlib.util
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("bench_long_audio", os.path.join(ROOT, "tools", "bench_long_audio.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rows = list(csv.DictReader(open(os.path.join(ROOT, "profiles", "r04_kernel_stats.csv"))))
    base = sum(float(r["TotalDurationNs"]) for r in rows)
    assert base > 0 and mod.share_of(rows)["share"] == 0
    names = {"frame_rms_kernel": "lds::frame_rms_kernel(float const*, float*, long long, int, int, int, int, long long, int, int)",
             "volume_kernel": "lds::volume_kernel(float const*, float*, long long, double, int, int, long long)",
             "volume_mask_kernel": "lds::volume_mask_kernel(float const*, float*, long long, int, float)",
             "resample_frames_ragged_kernel": "lds::resample_frames_ragged_kernel(float const*, float*, int, int, int, lds::RfLens)",
             "overlap_assemble_kernel": "lds::overlap_assemble_kernel(float const*, long long const*, int, float const*, float*, long long)"}
    assert set(names) == set(mod.NEW_KERNELS)
    for i, n in enumerate(names.values()):
        rows.append(dict(rows[0], Name=n, Calls=str(i + 1), TotalDurationNs=str(1000 * (i + 1))))
    got = mod.share_of(rows)
    assert got["per_kernel"]["volume_kernel"] == {"calls": 2, "us": 2.0} and got["per_kernel"]["volume_mask_kernel"] == {"calls": 3, "us": 3.0}
    assert abs(got["new_kernels_ms"] - 0.015) < 1e-12 and abs(got["share"] - 15000 / (base + 15000)) < 1e-12
