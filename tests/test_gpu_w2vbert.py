"""The w2v-BERT 2.0 units encoder on the GPU (include/lds.h lds_w2vbert_*, encoder.wav2vec2_bert.model, tools.tools.Wav2Vec2Bert /
Units_Encoder): the filter bank, the model on given features and the two in one against the fixtures recorded from transformers'
SeamlessM4TFeatureExtractor and Wav2Vec2BertModel (tests/golden/w2vbert.npz), every row of the long clips and a reduced configuration at
24 layers against the numpy restatement (tests/w2vbert_numpy.py, pinned to the same fixtures by tests/test_cpu_w2vbert.py), the three new
kernels alone, the ragged-batch invariants and the Python surface.  Weights: w2v-BERT 2.0's widths with 2 layers unless stated.

Bounds.  2e-5 x absmax against float64 is the project's bound for an fp32 encoder.  The front end takes a log (values near 20, whose fp32
spacing is 1.9e-6) and divides by a per-bin deviation over the clip's frames, so a short clip amplifies the rounding of the log itself: where
the fixture's recorded gap_feats (transformers' own extractor, which normalises in float32, against float64) is above 2e-6, the front-end
bound is 10 x that recorded gap instead -- a figure of the reference, never of the code under test."""
import os

import numpy as np
import pytest
import torch

import w2vbert_numpy as wnp
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

TOL = 2e-5              # x absmax against the fp64 reference
TOL_RAGGED = 1e-5       # x absmax: a clip inside a ragged batch against the clip alone, across buffer lengths
POISON = (0x7FC00000, 0x7F800000, 0xFF800000)      # NaN, +Inf, -Inf
SMALL = dict(n_mels=80, stride=2, n_state=128, n_head=2, n_ffn=256, n_layer=24, left_max=64, right_max=8, dw_kernel=31, n_ctx=1500, eps=1e-5)
RAGGED = (64240, 720, 560)
RAGGED_CLIPS = (4, 1, 0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def relmax(got, ref, absmax=None):
    return float(np.abs(got.astype(np.float64) - ref).max() / (absmax if absmax else max(np.abs(ref).max(), 1e-30)))


_Z, _STATE, _HANDLES, _CLIPS, _REF = {}, {}, {}, {}, {}


def fixtures():
    if not _Z:
        _Z.update(np.load(os.path.join(GOLDEN, "w2vbert.npz")))
    return _Z


def feats_tol(i):
    gap = float(fixtures()[f"gap_feats_{i}"])
    return 10.0 * gap if gap > 2e-6 else TOL


def _dims(small=False):
    from lds import arch
    return dict(SMALL) if small else dict(arch.W2V_BERT_DIMS, n_layer=wnp.FIXTURE_LAYERS)


def _state(small=False):
    from lds import arch
    if small not in _STATE:
        _STATE[small] = arch.w2vbert_init_state(_dims(small), wnp.FIXTURE_SEED)
    return _STATE[small]


def _handle(small=False):
    from lds import native
    if small not in _HANDLES:
        _HANDLES[small] = native.Wav2Vec2Bert(_dims(small), _state(small))
    return _HANDLES[small]


def _clip(i):
    from lds import init_weights
    if i not in _CLIPS:
        _CLIPS[i] = wnp.make_clip(i, init_weights.uniform)
    return _CLIPS[i]


def _numpy_ref(small, clip):
    """(input_features, encoder output) of the float64 restatement, computed once per (configuration, clip)"""
    key = (small, clip)
    if key not in _REF:
        f64 = wnp.fbank(_clip(clip))
        _REF[key] = (f64, wnp.encode(_state(small), _dims(small), f64, wnp.FRAMES[clip], np.float64))
    return _REF[key]


def test_w2vbert_fbank_encode_features_encode_vs_fixtures(record_margin):
    """lds_w2vbert_fbank against the extractor's input_features, lds_w2vbert_encode_features (on the restated features in fp32) and
    lds_w2vbert_encode against last_hidden_state: every recorded row of every fixture clip, the masked row of the odd clips included"""
    z, h = fixtures(), _handle()
    for i in range(len(wnp.CLIPS)):
        rows = z[f"rows_{i}"]
        a = dev(_clip(i)[None])
        fb = h.fbank(a)[0].cpu().numpy()
        assert fb.shape == (wnp.ROWS[i], 160) and np.isfinite(fb).all()
        e = relmax(fb[rows], z[f"feats_{i}"].astype(np.float64), float(z[f"absmax_feats_{i}"]))
        print(f"clip {i} fbank: {e:.3e} of absmax (bound {feats_tol(i):.1e}; the extractor's own gap {float(z[f'gap_feats_{i}']):.2e})")
        record_margin(e, feats_tol(i), f"feats{i}")
        if wnp.FRAMES[i] % 2:      # the masked row's second half is the extractor's padding
            assert not fb[-1, 80:].any()
        f32 = dev(wnp.fbank(_clip(i)).astype(np.float32)[None])
        for name, got in (("encf", h.encode_features(f32, [wnp.FRAMES[i]])), ("enc", h.encode(a))):
            got = got[0].cpu().numpy()
            assert got.shape == (wnp.ROWS[i], 1024) and np.isfinite(got).all()
            e = relmax(got[rows], z[f"enc_{i}"].astype(np.float64), float(z[f"absmax_enc_{i}"]))
            print(f"clip {i} {name}: {e:.3e} of absmax (the model's own fp32 gap {float(z[f'gap_enc_{i}']):.2e})")
            record_margin(e, TOL, f"{name}{i}")


def test_w2vbert_full_width_every_row_vs_numpy(record_margin):
    """the 75-, 76- and 200-row clips, of which the fixtures record selected rows only: every row against the float64 restatement"""
    h = _handle()
    for i in (2, 3, 4):
        f64, e64 = _numpy_ref(False, i)
        a = dev(_clip(i)[None])
        got_f, got_e = h.fbank(a)[0].cpu().numpy(), h.encode(a)[0].cpu().numpy()
        assert got_f.shape == f64.shape == (wnp.ROWS[i], 160) and got_e.shape == e64.shape == (wnp.ROWS[i], 1024)
        record_margin(relmax(got_f, f64), feats_tol(i), f"feats{i}")
        record_margin(relmax(got_e, e64), TOL, f"enc{i}")


def test_w2vbert_reduced_configuration_24_layers_vs_numpy(record_margin):
    """n_state 128, 2 heads, n_ffn 256, 24 layers: every row against the float64 restatement (an even and an odd clip)"""
    h = _handle(True)
    for i in (3, 4):
        _, e64 = _numpy_ref(True, i)
        assert 0.1 < np.abs(e64).max() < 100
        record_margin(relmax(h.encode(dev(_clip(i)[None]))[0].cpu().numpy(), e64), TOL, f"enc{i}")


def _ragged_audio(fill, L=None, lens=RAGGED, order=RAGGED_CLIPS):
    L = max(lens) if L is None else L
    a = np.full((len(lens), L), fill, dtype=np.float32)
    for b, (n, i) in enumerate(zip(lens, order)):
        a[b, :n] = _clip(i)[:n]
    return a


def test_w2vbert_ragged_vs_alone(record_margin):
    """B = 3 of 64,240 / 720 / 560 samples in one buffer, NaN beyond the clips: each against the clip alone (its own buffer length) within
    1e-5 absmax, rows beyond rows_b exactly zero"""
    h = _handle()
    audio = dev(_ragged_audio(np.nan))
    for what, call in (("feats", h.fbank), ("enc", h.encode)):
        got = call(audio, RAGGED)
        assert got.shape[:2] == (3, 200) and torch.isfinite(got).all()
        worst = 0.0
        for b, n in enumerate(RAGGED):
            R = wnp.frames_of(n)[2]
            alone = call(audio[b:b + 1, :n].contiguous())[0]
            worst = max(worst, relmax(got[b, :R].cpu().numpy(), alone.cpu().numpy().astype(np.float64)))
            assert not got[b, R:].any(), (what, b)
        record_margin(worst + 1e-30, TOL_RAGGED, what)


def test_w2vbert_same_buffer_length_is_bit_identical():
    """a clip alone in a buffer of L samples, inside B = 3 and inside B = 5 with the same L: the same bits (the tile rules are judged at
    the nominal batch); all lengths equal to L against lengths = NULL: the same bits"""
    h = _handle()
    L = max(RAGGED)
    lens5 = (560, 64240, 720, 24400, 560)
    a3 = dev(_ragged_audio(0.0))
    a5 = dev(_ragged_audio(0.0, L, lens5, (0, 4, 1, 3, 0)))
    u3, u5 = h.encode(a3, RAGGED), h.encode(a5, lens5)
    for b, n in enumerate(RAGGED):
        one = torch.zeros(1, L, device="cuda")
        one[0, :n] = a3[b, :n]
        alone = h.encode(one, [n])[0]
        assert torch.equal(u3[b], alone), b
        assert torch.equal(u5[(1, 2, 0)[b]], alone), b
    full = dev(np.stack([_clip(3), _clip(3)[::-1].copy()]))
    assert torch.equal(h.encode(full, [24400, 24400]), h.encode(full))
    assert torch.equal(h.fbank(full, [24400, 24400]), h.fbank(full))


def test_w2vbert_poison_changes_nothing():
    """NaN / 1e30 in the audio beyond lengths[b], a NaN / +Inf / -Inf workspace, five repeated calls: bit-identical to the clean run"""
    from lds import native
    h = _handle()
    clean = dev(_ragged_audio(0.0))
    ref, ref_f = h.encode(clean, RAGGED), h.fbank(clean, RAGGED)
    assert torch.isfinite(ref).all()
    for fill in (np.nan, 1e30):
        bad = dev(_ragged_audio(fill))
        assert torch.equal(h.encode(bad, RAGGED), ref) and torch.equal(h.fbank(bad, RAGGED), ref_f), fill
    bad = dev(_ragged_audio(np.nan))
    ws = torch.empty(h.workspace_bytes(3, max(RAGGED)), dtype=torch.uint8, device="cuda")
    for pat in POISON:
        native.debug_fill(ws, pat)
        assert torch.equal(h.encode(bad, RAGGED, ws=ws), ref), hex(pat)
        native.debug_fill(ws, pat)
        assert torch.equal(h.fbank(bad, RAGGED, ws=ws), ref_f), hex(pat)
        native.debug_fill(ws, pat)
        assert torch.equal(h.encode(bad[1:2, :720].contiguous(), ws=ws), h.encode(clean[1:2, :720].contiguous())), hex(pat)
    for _ in range(5):
        assert torch.equal(h.encode(bad, RAGGED), ref)


def test_w2vbert_short_clip_is_einval():
    """a 559-sample clip (one frame: the reference's variance is 0 / 0) is LDS_EINVAL from the C entry itself, before anything is enqueued"""
    from lds import native
    h = _handle()
    a = torch.zeros(1, 600, device="cuda")
    out = torch.empty(1, 1, 1024, device="cuda")
    ws = torch.empty(h.workspace_bytes(1, 600), dtype=torch.uint8, device="cuda")
    ln = np.array([559], dtype=np.int32)
    for entry in ("lds_w2vbert_encode", "lds_w2vbert_fbank"):
        rc = getattr(native.lib(), entry)(h.h, native._dev(a), native._host(ln), native._dev(out), native._dev(ws), ws.numel(), 1, 600, native._stream())
        assert rc == -1, (entry, rc)      # LDS_EINVAL
    assert native.lib().lds_w2vbert_encode(h.h, native._dev(a), None, native._dev(out), native._dev(ws), ws.numel(), 1, 559, native._stream()) == -1
    with pytest.raises(ValueError):
        h.encode(a, [559])


# ---- the three new kernels alone (include/lds_test.h) ------------------------------------------------------------------------------------
def _host_i32(v):
    return None if v is None else np.ascontiguousarray(v, dtype=np.int32)


# rows 1, 2, 31, 75 and 200 alone, and 200 next to a shorter ragged neighbour
def test_w2vbert_fbank_alone(record_margin):
    """w2vbert_fbank: 1 and 2 rows are fixture clips 0 and 1 (their recorded front-end bound), 31 / 75 / 200 rows prefixes of clip 4 and
    clips 2 and 4 against the float64 restatement; 200 rows next to a 75-row neighbour with NaN behind it"""
    from lds import native

    def run(audio, lens):
        B, L = audio.shape
        out = torch.full((B, wnp.frames_of(L)[2], 160), float("nan"), device="cuda")
        a, ln = dev(audio), _host_i32(lens)
        native.check(native.lib().lds_test_w2vbert_fbank(native._dev(a), native._host(ln), native._dev(out), B, L, native._stream()))
        return out.cpu().numpy()
    # (bound: a fixture clip's own; TOL for the prefix, which is no fixture clip and has no recorded gap)
    cases = [(feats_tol(0), _clip(0)), (feats_tol(1), _clip(1)), (TOL, _clip(4)[:400 + 160 * 61]), (feats_tol(2), _clip(2)), (feats_tol(4), _clip(4))]
    for tol, c in cases:
        got = run(c[None], None)[0]
        ref = wnp.fbank(c)
        assert got.shape == ref.shape and np.isfinite(got).all()
        record_margin(relmax(got, ref), tol, f"rows{ref.shape[0]}")
    both = np.full((2, 64240), np.nan, dtype=np.float32)
    both[0], both[1, :24240] = _clip(4), _clip(2)
    got = run(both, (64240, 24240))
    assert np.isfinite(got).all() and not got[1, 75:].any()
    record_margin(relmax(got[0], wnp.fbank(_clip(4))), TOL, "ragged200")
    record_margin(relmax(got[1, :75], wnp.fbank(_clip(2))), TOL, "ragged75")


ATT_CASES = [(1, 2, None, None), (2, 2, None, None), (2, 2, (2,), (1,)), (31, 2, None, None), (75, 2, (75,), (74,)), (200, 2, None, None),
             (200, 16, (200,), (199,)), (200, 2, (200, 75), (200, 74))]


def test_w2vbert_attention_alone(record_margin):
    """attention_k4p_rel + w2vbert_relpos: softmax((q.k + q.E[clamp(j - i, -64, 8) + 64]) / 8) v against float64 at every size at which the
    launcher takes another tile (32 rows, the 512-workgroup threshold at 200 rows x 16 heads), with fewer keys than queries (the masked
    row) and next to a shorter neighbour; zeros beyond a clip's queries whatever q and k hold there"""
    from lds import init_weights as iw, native
    for T, H, qr, kr in ATT_CASES:
        B, C = (1 if qr is None else len(qr)), 64 * H
        tag = f"t.w2vbert.att.{T}.{H}.{qr}"
        qkv = iw.uniform(tag + ".qkv", (B, 3 * C, T), 5, -1.2, 1.2)
        E = iw.uniform(tag + ".E", (73, 64), 5, -1.0, 1.0)
        if qr is not None:
            for b, n in enumerate(qr):      # (q and k hold anything beyond the clip; v holds the zeros its producer writes there)
                qkv[b, :2 * C, n:] = np.nan
                qkv[b, 2 * C:, n:] = 0.0
        out = torch.full((B, C, T), float("nan"), device="cuda")
        d = [dev(qkv), dev(E)]
        ql, kl = _host_i32(qr), _host_i32(kr)
        native.check(native.lib().lds_test_w2vbert_attention(native._dev(d[0]), native._dev(d[1]), native._host(ql), native._host(kl), native._dev(out),
                                                             B, C, T, H, 64, 8, native._stream()))
        got = out.cpu().numpy()
        assert np.isfinite(got).all()
        worst = 0.0
        for b in range(B):
            nq, nk = (T, T) if qr is None else (qr[b], kr[b])
            x = qkv[b, :, :nq].astype(np.float64)
            q, k, v = (x[i * C:(i + 1) * C].reshape(H, 64, nq).transpose(0, 2, 1) for i in range(3))
            ref = wnp.rel_attention(q, k, v, E, nk, 64, 8).transpose(0, 2, 1).reshape(C, nq)
            worst = max(worst, relmax(got[b, :, :nq], ref))
            assert not got[b, :, nq:].any()
        record_margin(worst, TOL, f"T{T}.H{H}.{'full' if qr is None else 'x'.join(map(str, kr))}")


DW_CASES = [(1, 64, None, None), (2, 1024, (2,), (1,)), (31, 1024, None, None), (75, 128, (75,), (74,)), (200, 1024, None, None),
            (200, 1024, (200, 76), (200, 75))]


def test_w2vbert_dwconv_alone(record_margin):
    """w2vbert_dwconv: causal depthwise convolution (31 taps) + LayerNorm over the channels + swish against float64; fewer input rows than
    output rows (the masked row reads as zero), more frames than the 30-frame left context, a shorter neighbour; zeros beyond a clip's rows"""
    from lds import init_weights as iw, native
    for T, C, orow, irow in DW_CASES:
        B = 1 if orow is None else len(orow)
        tag = f"t.w2vbert.dw.{T}.{C}.{orow}"
        x = iw.uniform(tag + ".x", (B, C, T), 6, -2.0, 2.0)
        w = iw.uniform(tag + ".w", (C, 31), 6, -0.31, 0.31)
        g, be = iw.uniform(tag + ".g", (C,), 6, 0.8, 1.2), iw.uniform(tag + ".be", (C,), 6, -0.1, 0.1)
        if orow is not None:
            for b, n in enumerate(irow):
                x[b, :, n:] = np.nan
        out = torch.full((B, C, T), float("nan"), device="cuda")
        d = [dev(v) for v in (x, w, g, be)]
        il, ol = _host_i32(irow), _host_i32(orow)
        native.check(native.lib().lds_test_w2vbert_dwconv(native._dev(d[0]), native._dev(d[1]), native._dev(d[2]), native._dev(d[3]), 1e-5, native._host(il),
                                                          native._host(ol), native._dev(out), B, C, T, 31, native._stream()))
        got = out.cpu().numpy()
        assert np.isfinite(got).all()
        worst = 0.0
        for b in range(B):
            no, ni = (T, T) if orow is None else (orow[b], irow[b])
            xb = np.nan_to_num(x[b, :, :no].astype(np.float64)).T
            ref = wnp.dwconv_ln_swish(xb, w.astype(np.float64), g.astype(np.float64), be.astype(np.float64), 1e-5, in_rows=ni).T
            worst = max(worst, relmax(got[b, :, :no], ref))
            assert not got[b, :, no:].any()
        record_margin(worst, TOL, f"T{T}.C{C}.{'full' if orow is None else 'x'.join(map(str, irow))}")


# ---- the Python surface -----------------------------------------------------------------------------------------------------------------
def test_w2vbert_units_encoder_encode_ragged_tokens(record_margin):
    import cluster
    from lds import init_weights
    from tools.tools import Units_Encoder, Wav2Vec2Bert
    enc = Units_Encoder("w2v-bert", model=Wav2Vec2Bert(dims=_dims(), state=_state()))
    assert enc.min_samples == 560 and enc.model.family == "w2v-BERT" and enc.model.n_ctx == 1500
    wav = dev(_clip(3))
    one = enc.encode(wav, 16000)
    assert one.shape == (76, 1024) and torch.equal(one, _handle().encode(wav[None])[0])
    short = enc.encode(wav[:250].contiguous(), 16000)      # zero-padded to 560 samples
    assert short.shape == (1, 1024) and torch.isfinite(short).all()
    batch = dev(_ragged_audio(np.nan))
    rag, n_rows = enc.encode_ragged(batch, RAGGED)
    assert n_rows.tolist() == [200, 2, 1] and rag.shape == (3, 200, 1024)
    alone = enc.encode(batch[1, :720].contiguous(), 16000)
    record_margin(relmax(rag[1, :2].cpu().numpy(), alone.cpu().numpy().astype(np.float64)) + 1e-30, TOL_RAGGED, "short")
    assert not rag[1, 2:].any()
    record_margin(relmax(rag[0].cpu().numpy(), enc.encode(batch[0].contiguous(), 16000).cpu().numpy().astype(np.float64)) + 1e-30, TOL_RAGGED, "long")
    m = enc.model.model      # the Wav2Vec2BertModel-shaped module: forward on features with the extractor's mask
    f = _handle().fbank(wav[None])
    mask = torch.ones(1, 76, dtype=torch.long)
    mask[0, 75] = 0
    assert torch.equal(m(f, mask), one[None]) and torch.equal(m.encode_audio(wav[None]), one[None])

    class Book:
        cluster_centers_ = init_weights.uniform("w2vbert.tokens.book", (64, 1024), 7, -1.0, 1.0)
    tok = enc.encode_tokens(wav, 16000, Book)
    assert tok.dtype == torch.int64 and torch.equal(tok, cluster.get_cluster_result(Book, one))
    tr, nf = enc.encode_tokens_ragged(dev(_ragged_audio(0.0)), RAGGED, Book, pad_id=-1)
    assert nf.tolist() == [200, 2, 1] and (tr[2, 1:] == -1).all() and (tr[2, :1] >= 0).all()
