"""The HuBERT units encoder on the GPU (include/lds.h lds_hubert_*, encoder.hubert.model, tools.tools.Units_Encoder): the feature
extractor and the transformer against the fixtures recorded from the reference (tests/golden/hubert.npz), a reduced configuration against
the numpy restatement (tests/hubert_numpy.py, pinned to the same fixtures by tests/test_cpu_hubert.py), the ragged-batch invariants and
the Python surface.  Weights: base widths with the first 2 layers (same seeded tensors as the 12-layer fixture model) unless stated."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import hubert_numpy as hnp
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

TOL = 2e-5              # x absmax against the fp64 reference: the project's bound for an fp32 encoder
TOL_RAGGED = 1e-5       # x absmax: a clip inside a ragged batch against the clip alone, across buffer lengths
POISON = (0x7FC00000, 0x7F800000, 0xFF800000)      # NaN, +Inf, -Inf
SMALL = dict(conv_dim=128, n_state=256, n_head=4, n_layer=2, n_ffn=512, n_proj=64, pos_kernel=128, pos_groups=16, n_ctx=1500)
RAGGED = (112077, 1279, 320)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def relmax(got, ref, absmax=None):
    return float(np.abs(got.astype(np.float64) - ref).max() / (absmax if absmax else max(np.abs(ref).max(), 1e-30)))


_Z = {}


def fixtures():
    if not _Z:
        _Z.update(np.load(os.path.join(GOLDEN, "hubert.npz")))
    return _Z


_STATE, _HANDLES, _CLIPS = {}, {}, {}


def _state(key, dims):
    from lds import arch
    if key not in _STATE:
        _STATE[key] = arch.hubert_init_state(dims, hnp.FIXTURE_SEED)
    return _STATE[key]


def _handle(layers=2, small=False):
    from lds import arch, native
    key = ("small" if small else "base", layers)
    if key not in _HANDLES:
        dims = dict(SMALL if small else arch.HUBERT_BASE_DIMS, n_layer=layers)
        _HANDLES[key] = native.Hubert(dims, _state(key, dims))
    return _HANDLES[key]


def _clip(i):
    from lds import init_weights
    if i not in _CLIPS:
        _CLIPS[i] = hnp.make_clip(i, init_weights.uniform)
    return _CLIPS[i]


def _against(name, i, got, record_margin):
    z = fixtures()
    ref, rows = z[f"{name}_{i}"].astype(np.float64), z[f"rows_{i}"]
    assert got.shape[0] == hnp.frames_of(hnp.CLIPS[i][0]) and got.shape[1] == ref.shape[1], (got.shape, ref.shape)
    assert np.isfinite(got).all()
    e = relmax(got[rows], ref, float(z[f"absmax_{name}_{i}"]))
    print(f"{name} clip {i}: max |native - ref64| / absmax {e:.3e} (reference's own fp32 gap {float(z[f'gap_{name}_{i}']):.2e})")
    record_margin(e, TOL, name)


@pytest.mark.parametrize("clip", [0, 1, 2, 3, 4])
def test_hubert_features_vs_reference(clip, record_margin):
    """lds_hubert_features: conv0 + norm0 + GELU and the six strided convolutions, every recorded row of every fixture clip"""
    got = _handle().features(dev(_clip(clip)[None]))[0].cpu().numpy()
    _against("feat", clip, got, record_margin)


@pytest.mark.parametrize("clip", [0, 1, 2, 3, 4])
def test_hubert_encode_layers_0_and_2_vs_reference(clip, record_margin):
    h = _handle()
    a = dev(_clip(clip)[None])
    _against("l0", clip, h.encode(a, layer=0)[0].cpu().numpy(), record_margin)
    _against("l2", clip, h.encode(a, layer=2)[0].cpu().numpy(), record_margin)


@pytest.mark.parametrize("clip", [0, 1, 2])
def test_hubert_full_depth_vs_reference(clip, record_margin):
    """all 12 layers: Hubert.encode and HubertSoft.units"""
    h = _handle(12)
    a = dev(_clip(clip)[None])
    _against("l12", clip, h.encode(a)[0].cpu().numpy(), record_margin)
    _against("units", clip, h.encode(a, proj=True)[0].cpu().numpy(), record_margin)


@pytest.mark.parametrize("clip", [1, 3])
def test_hubert_reduced_configuration_vs_numpy(clip, record_margin):
    """conv_dim 128, n_state 256, 16 groups of 16 channels (the base model's are 48 wide): every frame against the float64 restatement"""
    h = _handle(2, small=True)
    w = _state(("small", 2), dict(SMALL))
    audio = _clip(clip)
    f64 = hnp.features(w, audio, np.float64)
    a = dev(audio[None])
    record_margin(relmax(h.features(a)[0].cpu().numpy(), f64), TOL, "feat")
    for layer in (0, 2):
        ref = hnp.encode(w, SMALL, audio, layer=layer, dtype=np.float64, feats=f64)
        record_margin(relmax(h.encode(a, layer=layer)[0].cpu().numpy(), ref), TOL, f"l{layer}")
    ref = hnp.encode(w, SMALL, audio, proj=True, dtype=np.float64, feats=f64)
    record_margin(relmax(h.encode(a, proj=True)[0].cpu().numpy(), ref), TOL, "units")


@pytest.mark.parametrize("clip", [3, 4])
def test_hubert_base_width_every_frame_vs_numpy(clip, record_margin):
    """base widths (48-channel groups) on the 193- and 350-frame clips, of which the fixtures record selected rows only: every frame of
    the features, of `norm`'s output and of layer 2 against the float64 restatement (tests/test_cpu_hubert.py pins it to the fixtures'
    rows of these clips within 1e-6 absmax)"""
    from lds import arch
    h = _handle()
    dims = dict(arch.HUBERT_BASE_DIMS, n_layer=2)
    w = _state(("base", 2), dims)
    audio = _clip(clip)
    f64 = hnp.features(w, audio, np.float64)
    a = dev(audio[None])
    record_margin(relmax(h.features(a)[0].cpu().numpy(), f64), TOL, "feat")
    for layer in (0, 2):
        ref = hnp.encode(w, dims, audio, layer=layer, dtype=np.float64, feats=f64)
        got = h.encode(a, layer=layer)[0].cpu().numpy()
        assert got.shape == ref.shape == (hnp.CLIPS[clip][0] // 320, 768)
        record_margin(relmax(got, ref), TOL, f"l{layer}")


def _ragged_audio(fill, L=None, lens=RAGGED, order=(4, 1, 0)):
    L = max(lens) if L is None else L
    a = np.full((len(lens), L), fill, dtype=np.float32)
    for b, (n, i) in enumerate(zip(lens, order)):
        a[b, :n] = _clip(i)
    return a


def test_hubert_ragged_vs_alone(record_margin):
    """B = 3 of 112,077 / 1,279 / 320 samples in one buffer, NaN beyond the clips: each against the clip alone (its own buffer length)
    within 1e-5 absmax, rows beyond T_b exactly zero -- features, layer 2 and the transformer's input"""
    h = _handle()
    audio = dev(_ragged_audio(np.nan))
    for what, call in (("feat", lambda a, ln=None: h.features(a, ln)), ("l0", lambda a, ln=None: h.encode(a, ln, layer=0)),
                       ("l2", lambda a, ln=None: h.encode(a, ln, layer=2))):
        got = call(audio, RAGGED)
        assert got.shape[:2] == (3, 350) and torch.isfinite(got).all()
        worst = 0.0
        for b, n in enumerate(RAGGED):
            T = n // 320
            alone = call(audio[b:b + 1, :n].contiguous())[0]
            worst = max(worst, relmax(got[b, :T].cpu().numpy(), alone.cpu().numpy().astype(np.float64)))
            assert not got[b, T:].any(), (what, b)
        record_margin(worst, TOL_RAGGED, what)


def test_hubert_same_buffer_length_is_bit_identical():
    """a clip alone in a buffer of L samples, inside B = 3 and inside B = 5 with the same L: the same bits (the tile rules are judged at
    the nominal batch); all lengths equal to L against lengths = NULL: the same bits"""
    h = _handle()
    L = max(RAGGED)
    a3 = dev(_ragged_audio(0.0))
    a5 = dev(_ragged_audio(0.0, L, (320, 112077, 1279, 41277, 320), (0, 4, 1, 2, 0)))
    u3, u5 = h.encode(a3, RAGGED, layer=2), h.encode(a5, (320, 112077, 1279, 41277, 320), layer=2)
    for b, n in enumerate(RAGGED):
        one = torch.zeros(1, L, device="cuda")
        one[0, :n] = a3[b, :n]
        alone = h.encode(one, [n], layer=2)[0]
        assert torch.equal(u3[b], alone), b
        assert torch.equal(u5[(1, 2, 0)[b]], alone), b
    full = dev(np.stack([_clip(2), _clip(2)[::-1].copy()]))
    assert torch.equal(h.encode(full, [41277, 41277], layer=2), h.encode(full, layer=2))
    assert torch.equal(h.features(full, [41277, 41277]), h.features(full))


def test_hubert_poison_changes_nothing():
    """NaN / 1e30 in the audio beyond lengths[b], a NaN / +Inf / -Inf workspace, five repeated calls: bit-identical to the clean run"""
    from lds import native
    h = _handle()
    clean = dev(_ragged_audio(0.0))
    ref, ref_f = h.encode(clean, RAGGED, proj=True), h.features(clean, RAGGED)
    assert torch.isfinite(ref).all()
    for fill in (np.nan, 1e30):
        bad = dev(_ragged_audio(fill))
        assert torch.equal(h.encode(bad, RAGGED, proj=True), ref) and torch.equal(h.features(bad, RAGGED), ref_f), fill
    bad = dev(_ragged_audio(np.nan))
    ws = torch.empty(h.workspace_bytes(3, max(RAGGED)), dtype=torch.uint8, device="cuda")
    for pat in POISON:
        native.debug_fill(ws, pat)
        assert torch.equal(h.encode(bad, RAGGED, proj=True, ws=ws), ref), hex(pat)
        native.debug_fill(ws, pat)
        assert torch.equal(h.features(bad, RAGGED, ws=ws), ref_f), hex(pat)
        native.debug_fill(ws, pat)
        assert torch.equal(h.encode(bad[1:2, :1279].contiguous(), layer=1, ws=ws), h.encode(clean[1:2, :1279].contiguous(), layer=1)), hex(pat)
    for _ in range(5):
        assert torch.equal(h.encode(bad, RAGGED, proj=True), ref)


def _soft(layers=2):
    from encoder.hubert.model import HubertSoft
    from lds import arch
    dims = dict(arch.HUBERT_BASE_DIMS, n_layer=layers)
    m = HubertSoft(dims=dims)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in _state(("base", layers), dims).items()}, strict=True)
    return m.cuda().eval()


def test_hubert_python_surface(record_margin):
    """HubertSoft.units / encode / units_ragged and the two Units_Encoder names over the same handle's entries"""
    from tools.tools import HubertUnits, Units_Encoder
    m = _soft()
    wav = dev(_clip(2))
    u = m.units(wav.view(1, 1, -1))
    assert torch.equal(u, _handle().encode(wav[None], proj=True))
    padded = torch.nn.functional.pad(wav.view(1, 1, -1), (40, 40))
    x, none = m.encode(padded, layer=2)
    assert none is None
    _against("l2", 2, x[0].cpu().numpy(), record_margin)      # Hubert.encode takes the waveform as it is: the padded one gives the fixture
    batch = dev(_ragged_audio(np.nan))
    ur, nf = m.units_ragged(batch, RAGGED)
    assert nf.tolist() == [350, 3, 1] and torch.equal(ur, _handle().encode(batch, RAGGED, proj=True))
    state = _state(("base", 2), None)
    for name, width in (("hubertsoft", 256), ("contentvec768l12", 768)):
        enc = Units_Encoder(name, model=HubertUnits(name, dims=m.dims, state=state))
        one = enc.encode(wav, 16000)
        assert one.shape == (128, width) and torch.isfinite(one).all()
        rag, n_frames = enc.encode_ragged(batch, RAGGED)
        assert n_frames.tolist() == [350, 3, 1] and rag.shape == (3, 350, width)
        alone = enc.encode(batch[1, :1279].contiguous(), 16000)
        record_margin(relmax(rag[1, :3].cpu().numpy(), alone.cpu().numpy().astype(np.float64)), TOL_RAGGED, name)
        assert not rag[1, 3:].any()
        # the 112,077-sample row fills the buffer: 350 frames, more than one attention tile, the same buffer length on both sides
        long_alone = enc.encode(batch[0].contiguous(), 16000)
        assert long_alone.shape == (350, width)
        record_margin(relmax(rag[0].cpu().numpy(), long_alone.cpu().numpy().astype(np.float64)), TOL_RAGGED, name + ".long")
    assert torch.equal(Units_Encoder("hubertsoft", model=HubertUnits("hubertsoft", dims=m.dims, state=state)).encode(wav, 16000), u[0])


def test_hubert_encode_tokens_is_encode_plus_cluster():
    import cluster
    from lds import init_weights
    from tools.tools import HubertUnits, Units_Encoder
    m = _soft()
    enc = Units_Encoder("hubertsoft", model=HubertUnits("hubertsoft", dims=m.dims, state=_state(("base", 2), None)))

    class Book:
        cluster_centers_ = init_weights.uniform("hubert.tokens.book", (64, 256), 7, -1.0, 1.0)
    wav = dev(_clip(2))
    tok = enc.encode_tokens(wav, 16000, Book)
    assert tok.dtype == torch.int64 and torch.equal(tok, cluster.get_cluster_result(Book, enc.encode(wav, 16000)))
    batch = dev(_ragged_audio(0.0))
    tr, nf = enc.encode_tokens_ragged(batch, RAGGED, Book, pad_id=-1)
    units, _ = enc.encode_ragged(batch, RAGGED)
    assert torch.equal(tr, cluster.get_cluster_result(Book, units, lengths=nf, pad_id=-1)) and (tr[2, 1:] == -1).all()


def test_hubert_discrete_units_vs_numpy_argmin():
    """HubertDiscrete.units = encode(layer=7) + the nearest of 100 seeded centres; every frame is checked, and the inputs are such that
    the nearest and the second nearest centre differ by more than 1e-4 relative (verified here on the CPU, in float64)"""
    from encoder.hubert.model import HubertDiscrete
    from lds import arch, init_weights
    dims = dict(arch.HUBERT_BASE_DIMS, n_layer=7)
    state = arch.hubert_init_state(dims, hnp.FIXTURE_SEED, num_label_embeddings=504)

    class Book:
        cluster_centers_ = init_weights.uniform("hubert.discrete.book", (100, 768), 9, -1.5, 1.5)
    m = HubertDiscrete(Book, dims=dims)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    m = m.cuda().eval()
    wav = dev(_clip(2)).view(1, 1, -1)
    tok = m.units(wav)
    x = m.encode(torch.nn.functional.pad(wav, (40, 40)), layer=7)[0][0].cpu().numpy().astype(np.float64)
    d2 = ((x[:, None, :] - Book.cluster_centers_[None].astype(np.float64)) ** 2).sum(-1)
    srt = np.sort(d2, axis=1)
    assert ((srt[:, 1] - srt[:, 0]) / srt[:, 0]).min() > 1e-4      # no frame sits on a boundary: the arg-min is well defined for all 128
    assert tok.shape == (128,) and tok.dtype == torch.int64 and np.array_equal(tok.cpu().numpy(), d2.argmin(axis=1))


def test_extract_units_tool_hubertsoft(tmp_path):
    """tools/extract_units.py --synthetic --encoder hubertsoft on three generated clips writes three .npy files of the right shapes"""
    lens = [16000, 5000, 23456]
    for i, n in enumerate(lens):
        np.save(tmp_path / f"clip{i}.npy", _clip(2)[:n])
    out = tmp_path / "units"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "extract_units.py"), str(tmp_path), "--out", str(out), "--synthetic", "--layers", "2",
                        "--batch", "2", "--encoder", "hubertsoft"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for i, n in enumerate(lens):
        u = np.load(out / f"clip{i}.npy")
        assert u.shape == (n // 320, 256) and u.dtype == np.float32 and np.isfinite(u).all() and np.abs(u).max() > 0.1
