"""The x-vector speaker head on a real MI355X (csrc/xvector.hip through lds.native and encoder.xvector): one TDNN / linear layer against
float64 under the a-priori dot bound of tests/xvector_numpy.py, the pooling fused into the last layer against the float64 statistics of
the kernel's own fp32 output, the bit-for-bit invariances of an embedding, the weighted layer sum of the WavLM encoder, audio -> native
encoder -> head against transformers' WavLMForXVector (tests/golden/xvector.npz), the cosine kernel, the refusals that need a handle and
the tool."""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest

import wavlm_numpy as wnp
import xvector_numpy as XN
from conftest import ROOT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOL = 2e-5      # x absmax: tests/test_gpu_ctc.py's bound for audio -> encoder -> head; this head adds six dot products and one pooling
NAN = float("nan")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_layer(B, T, Cin, Cout, ks, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((B, T, Cin)).astype(np.float32)
    W = (rng.standard_normal((Cout, ks * Cin)) / np.sqrt(ks * Cin)).astype(np.float32)
    b = (rng.standard_normal(Cout) * 0.5).astype(np.float32)
    return X, W, b


def poison_beyond(X, n_frames):
    Xp = X.copy()
    for b, n in enumerate(n_frames):
        Xp[b, n:] = np.nan
    return Xp


# ---- one layer ----
LAYERS = ((64, 64, 1, 1), (64, 96, 5, 1), (128, 64, 3, 2), (64, 64, 3, 3), (512, 1500, 1, 1))
T_OUTS = ((1, 128, 300), (2, 127, 129))      # every T_out of {1, 2, 127, 128, 129, 300}, as two ragged batches of 3


def test_layer_against_float64(record_margin):
    """y against float64 under bound 1 at every (Cin, Cout, ks, d) x T_out: one frame, a full tile, one frame either side of it, three row
    blocks; Cout 96 and 1500 have tail column tiles (1500: 92 columns).  NaN sits behind every clip's n_frames and behind the output; rows
    from T_out to T are zeros.  ks 1 without ReLU is the projector."""
    from lds import native
    for Cin, Cout, ks, d in LAYERS:
        span, worst = (ks - 1) * d, 0.0
        for bi, touts in enumerate(T_OUTS):
            nf = [t + span for t in touts]
            B, T = 3, max(nf) + 5
            X, W, b = make_layer(B, T, Cin, Cout, ks, seed=Cin + Cout + 10 * ks + d + bi)
            relu = not (ks == 1 and Cin == Cout)
            flat = torch.full((B * T * Cout + 4096,), NAN, dtype=torch.float32, device="cuda")
            Y = native.xvector_test_tdnn(dev(poison_beyond(X, nf)), nf, dev(W), dev(b), ks, d, relu=relu, out=flat[:B * T * Cout].view(B, T, Cout))
            got, guard = Y.cpu().numpy(), flat[B * T * Cout:].cpu().numpy()
            assert np.isnan(guard).all()
            for c, (n, to) in enumerate(zip(nf, touts)):
                assert (got[c, to:] == 0).all(), (Cin, Cout, ks, d, to)
                ref = XN.tdnn(X[c, :n], W, b, ks, d, relu=relu)
                assert ref.shape == (to, Cout) and np.isfinite(got[c, :to]).all()
                worst = max(worst, float((np.abs(got[c, :to] - ref) / XN.delta_tdnn(X[c, :n], W, b, ks, d)).max()))
        print(f"layer Cin={Cin} Cout={Cout} ks={ks} d={d}: {worst:.3g} of bound 1")
        record_margin(worst, 1.0, f"{Cin}-{Cout}-{ks}-{d}")


def test_layer_zero_and_short_clips():
    """a clip too short for the kernel (T_out <= 0) and an empty one give all-zero rows and read nothing"""
    from lds import native
    X, W, b = make_layer(3, 40, 64, 64, 5, seed=1)
    nf = [4, 0, 40]
    Y = native.xvector_test_tdnn(dev(poison_beyond(X, nf)), nf, dev(W), dev(b), 5, 1).cpu().numpy()
    assert (Y[0] == 0).all() and (Y[1] == 0).all() and np.isfinite(Y[2]).all() and (Y[2, 36:] == 0).all() and np.abs(Y[2, :36]).max() > 0


# ---- the pooling in the last layer's epilogue ----
POOL_T_OUTS = ((2, 129, 1485), (3, 128, 257))


def pool_case(C, touts, seed):
    """(X, W, b, n_frames, ks, d): channel 0 constant (a zero weight row), channel 1 constant zero behind the ReLU, channel 2 with bias 1000 over
    unit-variance pre-activations"""
    Cin, ks, d = 64, (3 if C == 64 else 1), (2 if C == 64 else 1)
    nf = [t + (ks - 1) * d for t in touts]
    X, W, b = make_layer(3, max(nf) + 3, Cin, C, ks, seed)
    W[0], b[0] = 0.0, 0.37
    W[1], b[1] = 0.0, -1.0
    b[2] = 1000.0
    return X, W, b, nf, ks, d


def test_fused_pooling(record_margin):
    """(mean, std) of the fused kernel against the float64 statistics of the kernel's own fp32 output (the unfused mode's Y): mean within
    1e-5 and M2 within 1e-3, relative, at T_out 2, 3, one tile, one frame more, an odd number of 64-frame runs, 1485; C 64 and 1500.  A constant
    channel has a std of exactly 0 and its own value as the mean.  The bias-1000 channel separates Chan's combination (M2 to ~1e-6 relative)
    from E[x^2] - mean^2 (0.12)."""
    from lds import native
    for C in (64, 1500):
        wm, w2 = 0.0, 0.0
        for bi, touts in enumerate(POOL_T_OUTS):
            X, W, b, nf, ks, d = pool_case(C, touts, seed=C + bi)
            nbytes = native._bytes("lds_test_xvector_pool_workspace_bytes", 3, X.shape[1], C)
            ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            native.debug_fill(ws, 0x7fc07fc0)
            stats, Y = native.xvector_test_pool(dev(poison_beyond(X, nf)), nf, dev(W), dev(b), ks, d, return_y=True, ws=ws)
            stats, Y = stats.cpu().numpy(), Y.cpu().numpy()
            assert np.isfinite(stats).all()
            for c, to in enumerate(touts):
                mean, std = stats[c, :C].astype(np.float64), stats[c, C:].astype(np.float64)
                assert mean[0] == np.float32(0.37) and std[0] == 0.0 and mean[1] == 0.0 and std[1] == 0.0, (C, to, mean[:2], std[:2])
                m64, M2 = XN.pool_m2(Y[c, :to])
                const = (Y[c, :to] == Y[c, :1]).all(axis=0)      # (also channels whose few frames all sit behind the ReLU)
                assert const[0] and const[1] and (std[const] == 0).all() and (mean[const] == Y[c, 0, const]).all()
                live = ~const
                assert live[2] and live.sum() > C // 2 and (M2[live] > 0).all() and (m64[live] > 0).all()
                wm = max(wm, float((np.abs(mean - m64)[live] / m64[live]).max()))
                w2 = max(w2, float((np.abs(std ** 2 * (to - 1) - M2)[live] / M2[live]).max()))
                f2 = abs(std[2] ** 2 * (to - 1) - M2[2]) / M2[2]
                assert abs(m64[2] - 1000) < 1 and f2 < 1e-3, (C, to, f2)
                if to == 1485:
                    print(f"   C={C} T_out={to}: the bias-1000 channel's M2 is off by {f2:.2e} relative")
        print(f"pooling C={C}: mean {wm:.3g} (bound 1e-5), M2 {w2:.3g} (bound 1e-3), relative")
        record_margin(wm, 1e-5, f"mean-{C}")
        record_margin(w2, 1e-3, f"m2-{C}")


# ---- the head: invariances ----
def _head(D=768, n_layer=None):
    from encoder.xvector import XVectorHead
    return XVectorHead.synthetic(D, seed=XN.HEAD_SEED, n_layer=n_layer)


def test_embedding_bit_identity():
    """a clip's (embedding, logits) alone = the same clip at positions 0 and 2 of a ragged batch of 3 = with a larger Tmax and NaN behind it =
    on repeat = with a NaN-filled workspace; at 37 frames (one row block) and 300 (three, five pooling partials)"""
    from lds import native
    head = _head()
    rng = np.random.default_rng(7)
    other = rng.standard_normal((450, 768)).astype(np.float32)
    for n in (37, 300):
        clip = rng.standard_normal((n, 768)).astype(np.float32)
        base = [t.cpu().numpy() for t in head.embed(dev(clip[None]), [n])]
        assert np.isfinite(base[0]).all() and np.isfinite(base[1]).all() and base[0].shape == (1, 512)
        assert all(np.array_equal(a, t.cpu().numpy()) for a, t in zip(base, head.embed(dev(clip[None]), [n])))
        for T, lens in ((450, (n, 450, n)), (460, (n, 16, n)), (1499, (n, 20, n))):
            X = np.full((3, T, 768), np.nan, dtype=np.float32)
            X[0, :n], X[2, :n], X[1, :lens[1]] = clip, clip, other[:lens[1]]
            h = head.native()
            ws = torch.empty(native._bytes("lds_xvector_workspace_bytes", h.h, 3, T), dtype=torch.uint8, device="cuda")
            native.debug_fill(ws, 0x7fc07fc0)
            emb, logits = h.embed(dev(X), np.array(lens), ws=ws)
            emb, logits = emb.cpu().numpy(), logits.cpu().numpy()
            for at in (0, 2):
                assert np.array_equal(emb[at], base[0][0]) and np.array_equal(logits[at], base[1][0]), (n, T, at)
            assert np.isfinite(emb[1]).all()


def test_head_against_float64(record_margin):
    """the whole head on seeded hidden states against the float64 restatement: a ragged batch (16 frames = T_out 2, 129, 300) within TOL x absmax"""
    head = _head(1024)
    rng = np.random.default_rng(11)
    lens = (16, 129, 300)
    X = np.full((3, 310, 1024), np.nan, dtype=np.float32)
    for b, n in enumerate(lens):
        X[b, :n] = rng.standard_normal((n, 1024))
    emb, logits = (t.cpu().numpy() for t in head.embed(dev(X), lens))
    ref = [XN.head(head._state, X[b, :n]) for b, n in enumerate(lens)]
    e64, z64 = np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref])
    fe, fz = float(np.abs(emb - e64).max() / np.abs(e64).max()), float(np.abs(logits - z64).max() / np.abs(z64).max())
    print(f"head against float64: embeddings {fe:.2e}, logits {fz:.2e} of absmax (bound {TOL:g})")
    record_margin(max(fe, fz), TOL)


# ---- the layer sum ----
_STATE = {}


def _dims(flavour):
    from lds import arch
    return wnp.dims_of(flavour, arch)


def _state(flavour):
    from lds import arch
    if flavour not in _STATE:
        _STATE[flavour] = arch.wavlm_init_state(_dims(flavour), wnp.FIXTURE_SEED)
    return _STATE[flavour]


@pytest.mark.parametrize("flavour", wnp.FLAVOURS)
def test_layer_sum(flavour, record_margin):
    """lds_wavlm_encode_layersum against sum_l w_l lds_wavlm_encode(n_layers_run = l) formed in float64, bound 2 elementwise; two ragged clips
    (75 and 17 frames) with NaN behind them; rows beyond a clip are zeros; a repeat gives the same bits"""
    from lds import init_weights, native
    h = native.WavLM(_dims(flavour), _state(flavour))
    norm = flavour == "large"
    clips = [wnp.make_clip(2, init_weights.uniform), XN.make_clips(wnp, init_weights.uniform)[1]]
    lens = [len(c) for c in clips]
    audio = np.full((2, max(lens) + 100), np.nan, dtype=np.float32)
    for b, c in enumerate(clips):
        audio[b, :len(c)] = c
    w = XN.softmax(init_weights.uniform("xvector.layer_weights", (3,), 0, -1.0, 1.0)).astype(np.float32)
    a = dev(audio)
    got = h.encode(a, lens, normalize=norm, layer_weights=w)
    assert torch.equal(got, h.encode(a, lens, normalize=norm, layer_weights=w))
    got = got.cpu().numpy()
    hs = [h.encode(a, lens, layer=l, normalize=norm).cpu().numpy() for l in range(3)]
    ref = sum(np.float64(w[l]) * hs[l].astype(np.float64) for l in range(3))
    bound = XN.delta_layer_sum(hs, w)
    frames = [wnp.frames_of(n) for n in lens]
    assert frames == [75, 17]
    for b, n in enumerate(frames):
        assert (got[b, n:] == 0).all() and (bound[b, :n] > 0).all()
    valid = bound > 0
    assert (got[~valid] == 0).all()
    frac = float((np.abs(got - ref)[valid] / bound[valid]).max())
    print(f"layer sum {flavour}: {frac:.3g} of bound 2")
    record_margin(frac, 1.0)
    with pytest.raises(ValueError, match="3 finite numbers"):
        h.encode(a, lens, normalize=norm, layer_weights=[0.5, 0.5])
    with pytest.raises(ValueError, match="does not go with layer"):
        h.encode(a, lens, layer=1, normalize=norm, layer_weights=w)


# ---- end to end ----
@pytest.mark.parametrize("model", XN.MODELS)
def test_audio_to_embedding_against_transformers(model, golden, record_margin):
    """audio -> native WavLM -> head against WavLMForXVector in float64 (each clip alone, attention_mask None): the four fixture clips as ONE
    ragged batch with NaN behind every clip; embeddings and logits within TOL x absmax; the cosine matrix under bound 3 of its own inputs"""
    from encoder.xvector import SpeakerEncoder, XVectorHead
    from lds import arch, init_weights
    from tools.tools import WavLMUnits
    fx = golden("xvector.npz")
    flavour, use_sum = model.split("_")[0], model.endswith("_sum")
    name = "wavlmlarge" if flavour == "large" else "wavlmbase+"
    dims = _dims(flavour)
    units = WavLMUnits(name, dims=dims, state=_state(flavour))
    head = XVectorHead(arch.xvector_init_state(dims["n_state"], XN.HEAD_SEED, dims["n_layer"] if use_sum else None))
    spk = SpeakerEncoder(units, head)
    clips = XN.make_clips(wnp, init_weights.uniform)
    lens = [len(c) for c in clips]
    audio = np.full((4, max(lens) + 333), np.nan, dtype=np.float32)
    for b, c in enumerate(clips):
        audio[b, :len(c)] = c
    emb, logits = spk.embed_audio(dev(audio), lens, return_logits=True)
    cos = SpeakerEncoder.similarity(emb, emb).cpu().numpy()
    emb, logits = emb.cpu().numpy(), logits.cpu().numpy()
    am, gap = fx[f"{model}.absmax"], fx[f"{model}.gap"]
    fe = float(np.abs(emb - fx[f"{model}.embeddings"]).max() / am[0])
    fz = float(np.abs(logits - fx[f"{model}.logits"]).max() / am[1])
    print(f"{model}: embeddings {fe:.2e}, logits {fz:.2e} of absmax (bound {TOL:g}); transformers' own fp32 against its fp64: {gap[0]:.2e}, {gap[1]:.2e}; "
          f"cosine matrix off the fixture's by {np.abs(cos - fx[f'{model}.cosine']).max():.2e}")
    record_margin(max(fe, fz), TOL)
    assert np.abs(cos - XN.cosine(emb, emb)).max() <= XN.delta_cosine(512)
    with pytest.raises(ValueError, match="5199 samples gives 15 frames"):
        spk.embed_audio(dev(np.zeros((1, 5199), dtype=np.float32)))


# ---- the cosine kernel ----
def test_cosine_kernel(record_margin):
    from lds import native
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal((5, 512)).astype(np.float32), rng.standard_normal((7, 512)).astype(np.float32)
    b[3] = a[2] * 3.0      # a pair at cosine 1
    b[4] = 0.0             # a zero vector: 0 / (|a| 1e-8) = 0, not NaN
    got = native.xvector_cosine(dev(a), dev(b)).cpu().numpy()
    ref = XN.cosine(a, b)
    assert got.shape == (5, 7) and (got[:, 4] == 0).all()
    frac = float(np.abs(got - ref).max() / XN.delta_cosine(512))
    print(f"cosine [5, 512] x [7, 512]: {frac:.3g} of bound 3")
    record_margin(frac, 1.0)
    with pytest.raises(ValueError, match=r"\[N, dim\]"):
        native.xvector_cosine(dev(a), dev(b[:, :100]))


# ---- refusals that need a handle ----
def test_handle_refusals():
    from lds import arch, native
    lib = native.lib()
    g = dict(tdnn_dim=(64, 64), tdnn_kernel=(3, 1), tdnn_dilation=(2, 1), xvector_output_dim=32)
    st = arch.xvector_init_state(64, 0, None, 8, g)
    h = native.XVector(64, g["tdnn_dim"], g["tdnn_kernel"], g["tdnn_dilation"], 32, st)
    assert h.n_labels == 8 and h.span == 4
    with pytest.raises(RuntimeError, match=r"tdnn.1.kernel.bias \(absent\)"):
        native.XVector(64, g["tdnn_dim"], g["tdnn_kernel"], g["tdnn_dilation"], 32, {k: v for k, v in st.items() if k != "tdnn.1.kernel.bias"})
    with pytest.raises(RuntimeError, match=r"projector.weight \(wrong size\)"):
        native.XVector(96, g["tdnn_dim"], g["tdnn_kernel"], g["tdnn_dilation"], 32, st)
    X = torch.zeros(2, 20, 64, device="cuda")
    with pytest.raises(ValueError, match="5 frames leaves 1 frames to pool"):
        h.embed(X, [20, 5])
    nb = native._bytes("lds_xvector_workspace_bytes", h.h, 2, 20)
    emb, ws = torch.empty(2, 32, device="cuda"), torch.empty(nb, dtype=torch.uint8, device="cuda")
    call = lambda nf, Xp, ws_bytes: lib.lds_xvector_embed(h.h, Xp, nf.ctypes.data, native._dev(emb), None, native._dev(ws), ws_bytes, 2, 20, None)
    msg = lambda: lib.lds_last_error().decode()
    assert call(np.array([20, 5], dtype=np.int32), native._dev(X), nb) == -1 and "n_frames[1] = 5 gives 1 pooled frames" in msg() and "at least 6 frames" in msg()
    assert call(np.array([20, 6], dtype=np.int32), native._dev(X), nb - 1) == -2 and f"< {nb} bytes" in msg()
    assert call(np.array([20, 6], dtype=np.int32), None, nb) == -1 and "null pointer" in msg()
    assert call(np.array([20, 21], dtype=np.int32), native._dev(X), nb) == -1 and "n_frames[1] = 21" in msg()
    e, z = h.embed(X, [20, 6])
    assert torch.isfinite(e).all() and z.shape == (2, 8)


# ---- the tool ----
def test_tool_embed_and_verify(tmp_path):
    """tools/spk_eval.py --synthetic on three seeded clips (one a 22.05 kHz .wav: resampled on the device): one .npy per clip; verify prints a
    cosine per pair that equals the cosine of the embed files, a clip against itself gives 1, and labels give an EER"""
    import wave
    spec = importlib.util.spec_from_file_location("spk_eval", os.path.join(ROOT, "tools", "spk_eval.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rng = np.random.default_rng(3)
    clips = tmp_path / "clips"
    clips.mkdir()
    np.save(clips / "a.npy", (rng.standard_normal(9000) * 0.1).astype(np.float32))
    np.save(clips / "c.npy", (rng.standard_normal(6000) * 0.2).astype(np.float32))
    with wave.open(str(clips / "b.wav"), "wb") as w:
        w.setnchannels(1), w.setsampwidth(2), w.setframerate(22050)
        w.writeframes((rng.standard_normal(9000) * 3000).astype(np.int16).tobytes())
    common = ["--synthetic", "--layers", "1", "--encoder", "wavlmbase+"]
    out = tool.main(["embed", str(clips)] + common + ["--out", str(tmp_path / "emb")])
    emb = {n: np.load(os.path.join(out, n + ".npy")) for n in ("a", "b", "c")}
    assert all(e.shape == (512,) and e.dtype == np.float32 and np.isfinite(e).all() for e in emb.values())
    pairs = tmp_path / "pairs.txt"
    pairs.write_text("clips/a.npy clips/a.npy 1\nclips/a.npy clips/b.wav 0\nclips/c.npy clips/b.wav 0\n")
    res = json.load(open(tool.main(["verify", str(pairs)] + common)))
    got = [r["cosine"] for r in res["pairs"]]
    want = [XN.cosine(emb[x][None], emb[y][None])[0, 0] for x, y in (("a", "a"), ("a", "b"), ("c", "b"))]
    assert abs(got[0] - 1) <= XN.delta_cosine(512) and np.abs(np.array(got) - want).max() <= XN.delta_cosine(512)
    assert res["eer"] == 0.0 and got[1] < 1 and got[2] < 1
