"""The long-audio kernels on the GPU (csrc/svc.hip; include/lds.h lds_frame_rms, lds_volume_extract, lds_volume_mask,
lds_resample_frames_ragged, lds_overlap_assemble) against the float64 restatements of tests/svc_numpy.py.

Bounds (derived, not measured), u = 2^-24, gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1):

RMS and volume.  An fp32 evaluation squares n fp32 samples (one rounding each), adds the n squares in some fixed order (every partial sum
one rounding: at most n - 1 on the path of a term) and divides by n (one rounding): its mean square is sum x_i^2 (1 + e_i) with
|e_i| <= gamma_{n+1}.  The terms are nonnegative, so the error is relative: |ms' - ms| <= gamma_{n+1} ms.  The root halves a relative
error: sqrt(ms (1 + e)) = rms (1 + e / 2 + O(e^2)); the bound on the root is gamma_{n+1} / 2, relative, with n the frame length (for the
volume: the frame's own sample count).  That count leaves out the rounding of the root itself (u more), which decides at n = 3: a first
fp32 version of the kernels measured 1.04 of the bound at hop 3.5.  The kernels therefore sum in fp64 and round once, after the root:
their error is one fp32 rounding, u / (1 + u) < gamma_2 / 2 <= the bound at every n.  The float64 reference's own error, about
n 2^-53, is nine orders below.

Mask.  m and M are 0 or 1 exactly; f = (j % factor) / factor, 1 - f, two products and a sum: every operand lies in [0, 1], so the five
roundings are absolute errors of at most u / 2 each: 3 * 2^-24 covers them.

Assemble.  v = seg * mask (one rounding each for a and b); k = i / (F - 1) rounded once to fp32 (absolute error <= u / 2, which moves
k b and (1 - k) a by that much of |b| and |a|), 1 - k (one rounding), two products and a sum (one rounding each on values bounded by
|a| + |b|): |err| <= 5 u (|a| + |b|), about 3e-7 (|a| + |b|); outside an overlap one rounding of seg * mask, u |b|, or none without
a mask."""
import json
import os

import numpy as np
import pytest

import svc_numpy as SN
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def gamma(k):
    return k * U / (1 - k * U)


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "svc.npz"))), json.load(open(os.path.join(GOLDEN, "manifest_svc.json")))


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _signal(L, seed):
    """noise under a slow envelope from loud to 1e-4, fp32"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(L) * np.interp(np.arange(L), [0, max(L // 2, 1), max(L, 2)], [0.3, 1e-4, 0.2])).astype(np.float32)


def _worst_rel(got, ref, n):
    """(max of |got - ref| / ref, the smallest bound) after asserting every value within its own bound gamma_{n+1} / 2 (n: a count or one per
    value); a zero reference must be met exactly"""
    got, ref = got.astype(np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all()
    bound = np.broadcast_to(gamma(np.asarray(n, dtype=np.float64) + 1) / 2, ref.shape)
    assert np.array_equal(got[ref == 0], ref[ref == 0])
    nz = ref > 0
    if not nz.any():
        return 0.0, float(bound.min())
    rel = np.abs(got - ref)[nz] / ref[nz]
    assert (rel <= bound[nz]).all(), (float(rel.max()), float(bound[nz][np.argmax(rel / bound[nz])]))
    return float(rel.max()), float(bound.min())


# (13000, 3000) is not in the slicer's range: one frame exceeds the staging buffer there, the kernel's other path
@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
@pytest.mark.parametrize("fl,hop", [(1280, 320), (3528, 882), (5, 3), (13000, 3000)])
def test_frame_rms_against_float64(fl, hop, pad_mode, fx, record_margin):
    import torch
    from lds import native
    worst = 0.0
    for L in (1, fl // 2, fl - 1, fl, hop * 3 + 1, 85600):
        x = fx[0]["clip"] if (L == 85600 and fl == 1280) else _signal(L, L + fl)
        got = native.frame_rms(dev(x), fl, hop, pad_mode)
        again = native.frame_rms(dev(x), fl, hop, pad_mode)
        assert got.dtype == torch.float32 and got.is_cuda and got.shape == (SN.frame_rms_length(L, fl, hop),) and torch.equal(got, again)
        rel, bound = _worst_rel(got.cpu().numpy(), SN.frame_rms(x, fl, hop, pad_mode=pad_mode), fl)
        print(f"rms fl {fl} hop {hop} {pad_mode} L {L}: n {got.numel()}, worst relative error {rel:.3e} (bound {bound:.3e})")
        worst = max(worst, rel)
    # the relative error itself is recorded, in the same unit for every shape: one fp32 rounding whatever the frame length, while the
    # bound grows with it
    record_margin(worst + 1e-30, gamma(fl + 1) / 2)


@pytest.mark.parametrize("hop", [512.0, 512 * 16000 / 44100, 3.5], ids=["512", "185.76", "3.5"])
def test_volume_against_float64(hop, fx, record_margin):
    import torch
    from tools.tools import Volume_Extractor
    smallest = int((hop + 1) // 2) + 1
    worst, tightest = 0.0, np.inf
    for L in (smallest, smallest + 1, int(hop) * 3 + 1, 11000, 85600):
        x = fx[0]["clip"] if L == 85600 else _signal(L, L)
        ve = Volume_Extractor(hop_size=hop)
        got = ve.extract(dev(x))
        n = int(L // hop) + 1
        assert got.dtype == torch.float32 and got.is_cuda and got.shape == (n,) and torch.equal(got, ve.extract(x))      # (numpy goes to the device)
        Lp = L + int(hop // 2) + int((hop + 1) // 2)
        counts = [min(int((k + 1) * hop), Lp) - int(k * hop) for k in range(n)]
        rel, bound = _worst_rel(got.cpu().numpy(), SN.volume(x, hop), counts)      # (every frame within the bound of its own count)
        print(f"volume hop {hop:.2f} L {L}: n {n}, worst relative error {rel:.3e} (smallest bound {bound:.3e})")
        worst, tightest = max(worst, rel), min(tightest, bound)
    record_margin(worst + 1e-30, tightest)      # the relative error itself, against the bound of the shortest frame
    from lds import native
    with pytest.raises(RuntimeError, match="must exceed"):
        native.volume_extract(dev(_signal(smallest - 1, 1)), hop)
    # through the follow-the-input form the facade uses: hop = block_size * sr / model_sampling_rate
    ve = Volume_Extractor(hop_size=512, block_size=512, model_sampling_rate=44100)
    assert torch.equal(ve.extract(dev(fx[0]["clip"]), 16000), Volume_Extractor(hop_size=512 * 16000 / 44100).extract(dev(fx[0]["clip"])))


MASK_SLICES = {1: 50, 2: 51, 9: 46, 64: 20}      # n -> first frame of the fixture's hop-185.76 volume: every slice but n = 1 spans the first onset


@pytest.mark.parametrize("factor", [1, 7, 512])
@pytest.mark.parametrize("n", [1, 2, 9, 64])
def test_volume_mask_is_the_exact_formula(n, factor, fx):
    import torch
    from lds import native
    from tools.tools import Volume_Extractor
    vol = fx[0]["vol_1"][MASK_SLICES[n]: MASK_SLICES[n] + n].astype(np.float32)
    assert n < 9 or (vol.min() < 1e-3 and vol.max() > 0.05)      # (the slice spans the clip's first onset)
    worst = 0.0
    for db in (-60.0, -45.0, -20.0, -90.0):
        thr = np.float32(10 ** (db / 20))
        assert (np.abs(vol.astype(np.float64) - thr) >= 1e-3 * thr).all()
        got = native.volume_mask(dev(vol), factor, 10 ** (db / 20))
        assert got.shape == (n * factor,) and got.dtype == torch.float32
        want = SN.mask(vol, thr, factor)
        worst = max(worst, float(np.abs(got.cpu().numpy().astype(np.float64) - want).max()))
        if factor == 512:
            ve = Volume_Extractor(hop_size=512, block_size=512, model_sampling_rate=44100)
            m = ve.get_mask_from_volume(dev(vol), threhold=db, device="cuda")
            assert m.shape == (1, n * 512) and torch.equal(m[0], got)
    # (asserted here, not recorded among the parity margins: factors 1 and 512 are exact, so their zeros say nothing about factor 7)
    print(f"mask n {n} factor {factor}: worst |got - exact| {worst:.3e}")
    assert worst <= 3 * U


def test_volume_mask_against_the_reference_recording(fx, record_margin):
    """the recorded get_mask_from_volume (fp32 source positions: one spacing at position n <= 64, 64 * 2^-23 < 1e-5)"""
    from tools.tools import Volume_Extractor
    z, man = fx
    ve = Volume_Extractor(hop_size=512, block_size=512, model_sampling_rate=44100)
    worst = 0.0
    for j, db in enumerate(man["thresholds"]):
        got = ve.get_mask_from_volume(z["mask_in"].astype(np.float32), threhold=db, device="cuda")
        assert tuple(got.shape) == z[f"mask_{j}"].shape
        worst = max(worst, float(np.abs(got.cpu().numpy() - z[f"mask_{j}"]).max()))
    record_margin(worst + 1e-30, 1e-5)


def test_resample_frames_ragged_is_the_dense_entry_per_clip():
    import torch
    from lds import native
    from tools.tools import units_forced_alignment, units_forced_alignment_ragged
    rng = np.random.default_rng(2)
    B, Tin, Cc = 5, 37, 70
    tin, tout = [37, 1, 20, 9, 36], [50, 3, 7, 0, 300]
    x = rng.standard_normal((B, Tin, Cc)).astype(np.float32)
    for b in range(B):
        x[b, tin[b]:] = np.nan
    got = units_forced_alignment_ragged(dev(x), tin, tout)
    assert got.shape == (B, 300, Cc) and torch.isfinite(got).all()
    for b in range(B):
        assert not got[b, tout[b]:].any()
        if tout[b]:
            clip = dev(x[b:b + 1, :tin[b]])
            alone = native.resample_frames(clip, tout[b], float(np.float32(tin[b]) / np.float32(tout[b])))
            assert torch.equal(got[b:b + 1, :tout[b]], alone) and torch.equal(alone, units_forced_alignment(clip, n_frames=tout[b]))
    assert torch.equal(got, units_forced_alignment_ragged(dev(x), torch.tensor(tin), np.asarray(tout)))
    with pytest.raises(ValueError, match="lengths"):
        units_forced_alignment_ragged(dev(x), [38, 1, 20, 9, 36], tout)
    with pytest.raises(ValueError, match="at most 64"):
        units_forced_alignment_ragged(torch.zeros(65, 2, 4, device="cuda"), [2] * 65, [2] * 65)


# name -> (lengths, starts): gaps, exact abutment, overlaps of one sample (F = 1) and of a whole segment
ASSEMBLE = {
    "S1": ([300], [0]),
    "S1-leading-gap": ([300], [41]),
    "S2-gap": ([300, 200], [0, 517]),
    "S2-abut": ([300, 200], [7, 307]),
    "S2-F1": ([300, 200], [0, 299]),
    "S2-whole": ([300, 300], [5, 5]),
    "S2-whole-longer": ([1, 2000], [0, 0]),
    "S5": ([100, 50, 30, 40, 64], [0, 99, 149, 200, 200]),
    "S5-frames": ([512 * 9, 512 * 3, 512, 512 * 30, 512 * 2], [0, 512 * 8, 512 * 11, 512 * 11, 512 * 41]),
}


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("case", list(ASSEMBLE))
def test_overlap_assemble_against_the_sequential_loop(case, masked, record_margin):
    import torch
    from lds import native
    lens, starts = ASSEMBLE[case]
    rng = np.random.default_rng(len(case) + 7 * masked)
    segs = [rng.uniform(-1, 1, n).astype(np.float32) for n in lens]
    N = starts[-1] + lens[-1]
    mask = rng.uniform(0, 1, N + 5).astype(np.float32) if masked else None
    if masked:
        mask[N // 3: N // 3 + 40] = 0.0
    offset = np.concatenate([[0], np.cumsum(lens)[:-1]])
    packed = dev(np.concatenate(segs))
    got = native.overlap_assemble(packed, offset, starts, lens, None if mask is None else dev(mask))
    assert got.shape == (N,) and got.dtype == torch.float32
    for _ in range(3):
        assert torch.equal(got, native.overlap_assemble(packed, offset, starts, lens, None if mask is None else dev(mask)))
    want = SN.assemble(segs, starts, mask)
    mag = SN.assemble([np.abs(s) for s in segs], starts, None if mask is None else np.abs(mask))      # <= |a| + |b| ... and
    cover = np.zeros(N)
    both = np.zeros(N)
    for s, (n, st) in enumerate(zip(lens, starts)):
        v = np.abs(segs[s]).astype(np.float64) * (mask[st: st + n] if masked else 1.0)
        both[st: st + n] += v                                                                         # ... |a| + |b| itself
        cover[st: st + n] += 1
    assert cover.max() <= 2 and (mag <= both + 1e-12).all()
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    bound = np.where(cover == 2, 5 * U * both, (U * both) if masked else 0.0)
    assert (err[cover == 0] == 0).all() and (got.cpu().numpy()[cover == 0] == 0).all()
    assert (err <= bound).all(), (case, float(err.max()), int(np.argmax(err - bound)))
    nz = bound > 0
    record_margin(float((err[nz] / bound[nz]).max()) + 1e-30 if nz.any() else 1e-30, 1.0)


def test_overlap_assemble_preconditions_and_cross_fade(fx):
    import torch
    from lds import native
    from tools.tools import cross_fade
    z, man = fx
    for k, idx in enumerate(man["cross_fades"]):
        a, b, ref = z[f"xf_{k}_a"], z[f"xf_{k}_b"], z[f"xf_{k}_out"]
        got = cross_fade(a.astype(np.float32), dev(b.astype(np.float32)), idx)
        assert got.is_cuda and got.shape == ref.shape
        a32, b32 = np.abs(a.astype(np.float32)).astype(np.float64), np.abs(b.astype(np.float32)).astype(np.float64)
        F = len(a) - idx
        bound = np.zeros(len(ref))
        bound[idx: idx + F] = 5 * U * (a32[idx:] + b32[:F])
        want = SN.assemble([a.astype(np.float32), b.astype(np.float32)], [0, idx])
        assert (np.abs(got.cpu().numpy() - want) <= bound).all()
        assert np.abs(want - ref).max() < 1e-7      # (the recording took the float64 clip: within the inputs' fp32 rounding of it)
    segs = torch.zeros(60, device="cuda")
    for off, start, ln, msg in [([0, 10], [6, 5], [10, 10], "segment 1: start 5 below"), ([0, 10], [0, 2], [10, 3], "segment 1: the overlap"),
                                ([0, 10, 30], [0, 7, 8], [10, 20, 30], "segment 2: start 8 inside segment 0")]:
        with pytest.raises(ValueError, match=msg):
            native.overlap_assemble(segs, off, start, ln)
    with pytest.raises(ValueError, match="the mask holds 19"):
        native.overlap_assemble(segs, [0, 10], [0, 10], [10, 10], torch.ones(19, device="cuda"))
    with pytest.raises(ValueError, match="a mono 1-D waveform"):
        native.frame_rms(torch.zeros(2, 100, device="cuda"), 16, 4)
