"""DiffusionSVC.infer_from_long_audio with a 2-layer HuBERT-Soft units encoder on a short three-segment recording, mirroring
tests/test_gpu_svc.py's checks and tolerances (its helpers are used as they are): the method against the hand-written composition of the
public ragged entries within the join's bound, and batch_size 1 against 3 within four times the discrepancy between the dense per-segment
chain (each segment through its stand-alone encode / align / infer) and the ragged chain, measured in the same session."""
import os

import numpy as np
import pytest

import test_gpu_svc as TS
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
KW = TS.KW


@pytest.fixture(scope="module")
def svc():
    import infer_svc
    return infer_svc.synthetic_svc("cuda", layers=2, encoder="hubertsoft")


@pytest.fixture(scope="module")
def clip(svc):
    """the first three segments of the long-audio fixture's recording"""
    full = TS.dev(np.load(os.path.join(GOLDEN, "svc.npz"))["clip"])
    ranges, _ = TS._segments(svc, full, 16000)
    cut = full[:(ranges[2][2] + ranges[3][1]) // 2].contiguous()
    assert len(TS._segments(svc, cut, 16000)[0]) == 3
    return cut


def test_hubert_long_audio_is_the_composition_of_the_ragged_entries(svc, clip, record_margin):
    import torch
    assert svc.units_encoder.encoder == "hubertsoft" and svc.units_encoder.min_samples == 320
    ranges, n_frames = TS._segments(svc, clip, 16000)
    x_T = TS._noise(n_frames, 5)
    got, rate = svc.infer_from_long_audio(clip, sr=16000, batch_size=3, x_T=x_T, **KW)
    assert rate == 44100 and got.is_cuda and got.dtype == torch.float32 and torch.isfinite(got).all()
    chunks = [sorted(range(3), key=lambda s: ranges[s][2] - ranges[s][1])]
    rows = TS._ragged_rows(svc, clip, 16000, ranges, n_frames, x_T, chunks)
    mask = svc.extract_volume_and_mask(clip, 16000, threhold=-60.0)[1][0].cpu().numpy()
    record_margin(TS._join_check(got.cpu().numpy(), rows, ranges, n_frames, mask) + 1e-30, 1.0)
    units, frames = svc.units_encoder.encode_ragged(clip[None, ranges[0][1]:ranges[0][2]].contiguous(), [ranges[0][2] - ranges[0][1]])
    assert int(frames[0]) == (ranges[0][2] - ranges[0][1]) // 320 and units.shape[-1] == 256      # the HuBERT frame rule


def test_hubert_batch_size_1_against_3_under_one_seed(svc, clip, record_margin):
    import torch
    parent = TS.parent_chain_discrepancy(svc, clip)      # every segment's stand-alone chain against the ragged chain
    outs = []
    for bs in (1, 3):
        torch.manual_seed(1234)
        outs.append(svc.infer_from_long_audio(clip, sr=16000, batch_size=bs, **KW)[0])
    assert outs[0].shape == outs[1].shape
    diff = float((outs[0] - outs[1]).abs().max() / outs[0].abs().max())
    print(f"dense chain against ragged chain: {parent:.3e}; batch_size 1 against 3: {diff:.3e}")
    assert parent > 0
    record_margin(diff + 1e-30, 4 * parent)
    torch.manual_seed(1234)
    assert torch.equal(svc.infer_from_long_audio(clip, sr=16000, batch_size=3, **KW)[0], outs[1])      # a repeat: the same bits
