"""The epilogues of the transformer's two LayerNorm-folded projections as the UNet launches them (csrc/conv_dma.hip):

  * QKV: fold, bias and the value split in ONE launch.  Single-tile waves fetch the fold's row constants through late_loads() (ln_c1 in the
    residual slots, ln_c2 in the bias quads); the value rows leave in the attention's VT layout (store_vt).
  * FF1: fold + GEGLU on two-tile waves, whose constants arrive as 16-byte loads (row_consts).

Every case fills the outputs with NaN and checks EVERY element against a float64 numpy computation at 2e-5 of max|ref| (the bound
tests/test_gpu_store16.py holds the same entry point to); the VT tail (frames T .. ceil4(T) - 1) and the frames at and beyond a ragged
length must be exactly zero, and nothing may be left NaN.  The K4P buffer is read through lds_test_tap_k4p as well.

Bit identity needs no second library: with the same weight rows, LayerNorm constants and bias in the q third and in the v third, the value
read back from VT must equal the q value read from K4P bit for bit, whatever form the value store has.  (The transposed-tile form it was
written for was measured inside the A/B's spread and taken out again; with it went the configuration tag that
named it, so no tag is asserted here.  This test is what found that the fold expression was rounded differently in different kernels.)

Shapes: B = 2; C in {64, 96, 128} with two heads (D = 32, 48, 64: 48 puts a head boundary inside a tile, 96 ends the rows inside an M-block);
Ci in {64, 128} = 4 and 8 K-steps through the BK 16 x 3-deep ring; T in {37, 64, 130} (a ragged block with T % 4 = 1, one full block,
several blocks), dense and with lens = [T, T - 33]."""
import ctypes as ct

import numpy as np
import pytest

from test_gpu_store16 import D, Tap, U as U16, check_all, conv64, dev, masked, nan_out, stream

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

QKV_CFG = 64064163      # the UNet's QKV tile: 64 x 64, BK 16, 3-deep ring


def U(name, shape, lo=-1.0, hi=1.0):
    return U16("qe." + name, shape, lo, hi)


def ln64(x, g, be, eps=1e-5):
    x = x.astype(np.float64)
    mu, var = x.mean(1, keepdims=True), x.var(1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * g[None, :, None] + be[None, :, None]


def run_qkv(x, w, b, g, be, Dh, cfg=0, lengths=None, tile_batch=0):
    """-> (q;k [B][2C][T], v [B][C][ceil4(T)] read back from VT, configuration string)"""
    from lds import native
    B, Ci, T = x.shape
    C3 = w.shape[0]
    C = C3 // 3
    T4 = (T + 3) // 4 * 4
    a = native.DConvExTest()
    dx = dev(x)
    wk, bk = np.ascontiguousarray(w, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    ln_i = np.asarray(lengths, dtype=np.int32) if lengths is not None else None
    a.x1, a.x2, a.C1, a.C2, a.T = dx.data_ptr(), None, Ci, 0, T
    a.w, a.bias, a.Co, a.K, a.stride, a.pad = wk.ctypes.data, bk.ctypes.data, C3, 1, 1, 0
    a.res, a.epilogue = None, 0
    a.lengths, a.lvl_in, a.lvl_out = (ln_i.ctypes.data if ln_i is not None else None), 0, 0
    a.ln_gamma, a.ln_beta, a.ln_eps = g.ctypes.data, be.ctypes.data, 1e-5
    a.tile_batch, a.fmt, a.v_split, a.cfg = tile_batch, -1, Dh, cfg
    out = nan_out(B * 2 * C * T + B * C * T4)
    cfg_s = ct.create_string_buffer(160)
    with Tap(B, 2 * C, T) as tap:
        native.check(native.lib().lds_test_dconv_ex(ct.byref(a), D(out), None, B, cfg_s, len(cfg_s), stream()))
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    qk = o[:B * 2 * C * T].reshape(B, 2 * C, T)
    tap.check(qk)
    vt = o[B * 2 * C * T:].reshape(B, C // Dh, T4 // 4, Dh, 4).transpose(0, 1, 3, 2, 4).reshape(B, C, T4)
    print(f"  {cfg_s.value.decode()}")
    return qk, vt, cfg_s.value.decode()


def qkv_case(C, Ci, T, tag):
    x = U(f"{tag}.x", (2, Ci, T), -2, 2) + np.float32(0.3)
    w = U(f"{tag}.w", (3 * C, Ci, 1)) / np.float32(np.sqrt(Ci))
    b = U(f"{tag}.b", (3 * C,))
    g, be = U(f"{tag}.g", (Ci,), 0.5, 1.5), U(f"{tag}.be", (Ci,), -0.5, 0.5)
    return x, w, b, g, be


def check_qkv(qk, vt, ref, C, T, lengths=None):
    assert np.isfinite(vt).all(), "an element of the VT buffer was left NaN"
    assert (vt[:, :, T:] == 0).all(), "VT tail not zero"
    check_all(qk, ref[:, :2 * C], lengths=lengths)
    check_all(vt[:, :, :T], ref[:, 2 * C:], lengths=lengths)


@pytest.mark.parametrize("T", [37, 64, 130])
@pytest.mark.parametrize("Ci", [64, 128])
@pytest.mark.parametrize("C", [64, 96, 128])
def test_qkv_fold_bias_value_split(C, Ci, T):
    """the real QKV combination on the UNet's QKV tile, dense and ragged"""
    x, w, b, g, be = qkv_case(C, Ci, T, f"q{C}.{Ci}.{T}")
    qk, vt, cfg = run_qkv(x, w, b, g, be, C // 2, cfg=QKV_CFG)
    assert cfg.startswith("BM64 BN64 KT1 S1 U0 BK16 NST3"), cfg
    check_qkv(qk, vt, conv64(ln64(x, g, be), w, b), C, T)
    lengths = [T, T - 33]
    xm = masked(x, lengths)
    qk, vt, cfg = run_qkv(xm, w, b, g, be, C // 2, cfg=QKV_CFG, lengths=lengths)
    check_qkv(qk, vt, masked(conv64(ln64(xm, g, be), w, b), lengths), C, T, lengths=lengths)


@pytest.mark.parametrize("T", [37, 130])
@pytest.mark.parametrize("C", [64, 128])
def test_value_rows_bit_identical_to_query_rows(C, T):
    """the same rows, constants and bias in the q third and in the v third: VT == K4P, bit for bit"""
    x, w, b, g, be = qkv_case(C, 64, T, f"bit{C}.{T}")
    w[2 * C:], b[2 * C:] = w[:C], b[:C]
    qk, vt, cfg = run_qkv(x, w, b, g, be, C // 2, cfg=QKV_CFG)
    assert np.isfinite(vt).all() and (vt[:, :, T:] == 0).all()
    assert np.array_equal(vt[:, :, :T], qk[:, :C]), "the value rows differ from the same query rows"
    check_all(qk, conv64(ln64(x, g, be), w, b)[:, :2 * C])


def test_qkv_auto_tile():
    """the tile the launcher picks by itself for a small QKV (its own rules, no forced configuration): all values, whatever form ran"""
    C, T = 128, 70
    x, w, b, g, be = qkv_case(C, 64, T, "auto")
    qk, vt, _ = run_qkv(x, w, b, g, be, C // 2)
    check_qkv(qk, vt, conv64(ln64(x, g, be), w, b), C, T)


@pytest.mark.parametrize("T", [37, 130])
def test_wide_qkv_two_tile_waves(T):
    """a 128 x 64-tile QKV at C = 128 (forced): two-tile waves, row constants as 16-byte loads, value rows through store_vt"""
    C = 128
    x, w, b, g, be = qkv_case(C, 64, T, f"wide.{T}")
    qk, vt, cfg = run_qkv(x, w, b, g, be, C // 2, cfg=128064322)
    assert cfg.startswith("BM128 BN64"), cfg
    check_qkv(qk, vt, conv64(ln64(x, g, be), w, b), C, T)


def test_latency_mode_cluster_split():
    """B = 1 in latency mode on a QKV that cluster-splits (Ci = 256: the 32 x 64 split-K tile, four K-steps of BK 64 shared by two
    workgroups): every workgroup fetches the fold's constants through its late loads, one leaves in cluster_join, the other applies them"""
    C, Ci, T = 64, 256, 64
    x = U("lat.x", (1, Ci, T), -2, 2) + np.float32(0.3)
    w = U("lat.w", (3 * C, Ci, 1)) / np.float32(np.sqrt(Ci))
    b = U("lat.b", (3 * C,))
    g, be = U("lat.g", (Ci,), 0.5, 1.5), U("lat.be", (Ci,), -0.5, 0.5)
    qk, vt, cfg = run_qkv(x, w, b, g, be, C // 2, tile_batch=1)
    assert " KS" in cfg, cfg
    check_qkv(qk, vt, conv64(ln64(x, g, be), w, b), C, T)


@pytest.mark.parametrize("T", [37, 130])
def test_ff1_fold_geglu(T):
    """FF1: 64 -> 512 rows, LayerNorm fold + value * gelu(gate) on 128-row tiles"""
    from math import erf
    from lds import native
    B, Ci = 2, 64
    x = U(f"ff{T}.x", (B, Ci, T), -2, 2) + np.float32(0.3)
    w, b = U(f"ff{T}.w", (512, Ci, 1)) / np.float32(8), U(f"ff{T}.b", (512,))
    g, be = U(f"ff{T}.g", (Ci,), 0.5, 1.5), U(f"ff{T}.be", (Ci,), -0.5, 0.5)
    a = native.DConvExTest()
    dx = dev(x)
    wk, bk = np.ascontiguousarray(w, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    a.x1, a.x2, a.C1, a.C2, a.T = dx.data_ptr(), None, Ci, 0, T
    a.w, a.bias, a.Co, a.K, a.stride, a.pad = wk.ctypes.data, bk.ctypes.data, 512, 1, 1, 0
    a.res, a.epilogue, a.lengths, a.lvl_in, a.lvl_out = None, 1, None, 0, 0
    a.ln_gamma, a.ln_beta, a.ln_eps = g.ctypes.data, be.ctypes.data, 1e-5
    a.tile_batch, a.fmt, a.v_split, a.cfg = 0, -1, 0, 0
    out = nan_out(B, 256, T)
    cfg = ct.create_string_buffer(160)
    with Tap(B, 256, T) as tap:
        native.check(native.lib().lds_test_dconv_ex(ct.byref(a), D(out), None, B, cfg, len(cfg), stream()))
    torch.cuda.synchronize()
    print(f"  {cfg.value.decode()}")
    assert cfg.value.decode().startswith("BM128"), cfg.value
    got = out.cpu().numpy()
    tap.check(got)
    y = conv64(ln64(x, g, be), w, b)
    val, gate = y[:, :256], y[:, 256:]
    check_all(got, val * 0.5 * gate * (1 + np.vectorize(erf)(gate / np.sqrt(2.0))))

