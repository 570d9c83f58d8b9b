"""conv2 + shortcut as one Winograd reduction, the parts that need no GPU: the restatement of tests/wino_pair_numpy.py against
the direct conv2 + shortcut in float64 (dense, odd and ragged), in fp32 GEMMs against float64 at the UNet's widths, and the library's host-side
pack (lds_test_wino_pair_pack) against the float64 transform rounded once."""
import ctypes as ct

import numpy as np
import pytest

import wino_numpy as W
import wino_pair_numpy as WP


def U(name, shape, lo=-1.0, hi=1.0):
    from lds import init_weights
    return init_weights.uniform("wino.pair.cpu." + name, shape, 30, lo, hi)


def make(tag, Cin, Cm, T):
    d, x = U(tag + ".d", (Cm, T), -2, 2), U(tag + ".x", (Cin, T), -2, 2)
    g = U(tag + ".g", (Cm, Cm, 3)) / np.float32(np.sqrt(3 * Cm))
    S = U(tag + ".S", (Cm, Cin)) / np.float32(np.sqrt(Cin))
    return d, x, g.astype(np.float32), S.astype(np.float32)


@pytest.mark.parametrize("Cin,Cm,T", [(32, 32, 7), (64, 32, 1), (64, 96, 64), (32, 96, 65), (256, 384, 65)])
def test_pair_equals_direct_float64(Cin, Cm, T):
    d, x, g, S = make(f"eq{Cin}.{Cm}.{T}", Cin, Cm, T)
    got, ref = WP.pair_conv(d, x, g, S), WP.pair_direct(d, x, g, S)
    assert got.shape == ref.shape == (Cm, T)
    assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("T,length", [(130, 37), (65, 64), (64, 1), (7, 7)])
def test_pair_ragged_zero_rule(T, length):
    """NaN / Inf at and beyond the length reach no plane; the result is the utterance alone; zeros beyond"""
    Cin, Cm = 64, 32
    d, x, g, S = make(f"rg{T}.{length}", Cin, Cm, T)
    bd, bx = d.copy(), x.copy()
    bd[:, length:] = np.nan
    bx[:, length:] = np.where(np.arange(T - length) % 2 == 0, np.nan, np.inf)
    V = WP.pair_planes(bd, bx, length)
    assert V.shape == (4, Cm + Cin // 2, (T + 1) // 2) and np.isfinite(V).all()
    assert np.array_equal(V[:, Cm:, :(length + 1) // 2], WP.side_planes(x[:, :length]))
    assert not V[:, Cm:, (length + 1) // 2:].any()
    got = WP.pair_conv(bd, bx, g, S, length)
    alone = WP.pair_direct(d[:, :length], x[:, :length], g, S)
    assert np.isfinite(got).all() and not got[:, length:].any()
    assert np.abs(got[:, :length] - alone).max() <= 1e-12 * max(1.0, np.abs(alone).max())


@pytest.mark.parametrize("Cin,Cm,T", [(1024, 512, 64), (640, 256, 130), (256, 384, 65), (32, 32, 7)])
def test_pair_fp32_gemms_against_float64(Cin, Cm, T):
    """the form as the GPU runs it -- fp32 taps, fp32 planes, fp32 products, fp32 join -- against the float64 direct sum of the same fp32
    inputs: inside the kernels' bound of 1e-5"""
    d, x, g, S = make(f"f32.{Cin}.{Cm}.{T}", Cin, Cm, T)
    Uf, V = WP.pair_taps_f32(g, S), WP.pair_planes(d, x)
    assert V.dtype == np.float32
    M = np.stack([Uf[j] @ V[j] for j in range(4)])
    assert M.dtype == np.float32
    Y = np.empty((Cm, 2 * V.shape[-1]), dtype=np.float32)
    Y[:, 0::2] = (M[0] + M[1]) + M[2]
    Y[:, 1::2] = (M[1] - M[2]) - M[3]
    ref = WP.pair_direct(d, x, g, S)
    assert np.abs(Y[:, :T] - ref).max() / np.abs(ref).max() < 1e-5


def test_side_planes_are_single_fp32_operations():
    x = U("side", (32, 5), -2, 2)
    V = WP.side_planes(x)
    assert V.dtype == np.float32 and V.shape == (4, 16, 3)
    assert np.array_equal(V[0, :, 1], x[:16, 2]) and np.array_equal(V[3, :, 1], x[:16, 3])
    assert np.array_equal(V[1, :, 0], x[16:, 0] + x[16:, 1]) and np.array_equal(V[2, :, 0], x[16:, 0] - x[16:, 1])
    # frame T of an odd T does not exist: x_o of the last pair is zero
    assert not V[3, :, 2].any() and np.array_equal(V[1, :, 2], x[16:, 4]) and np.array_equal(V[2, :, 2], x[16:, 4])


@pytest.mark.parametrize("Co,Cm,Cin", [(1, 1, 2), (32, 32, 32), (96, 96, 64)])
def test_pair_pack_matches_float64_transform(Co, Cm, Cin):
    from lds import native
    g, S = U(f"pk.g{Co}.{Cin}", (Co, Cm, 3), -3, 3), U(f"pk.S{Co}.{Cin}", (Co, Cin), -3, 3)
    g[0, 0] = [1.0, 2.0 ** -24, -1.0]      # (not representable after an fp32 sum: the pack rounds once)
    S[0, Cin // 2] = np.float32(2.0 ** -126)      # halving a normal number at the bottom of the range stays exact (a subnormal)
    out = np.full((4, Co, Cm + Cin // 2), np.nan, dtype=np.float32)
    native.check(native.lib().lds_test_wino_pair_pack(ct.c_void_p(g.ctypes.data), ct.c_void_p(S.ctypes.data), Co, Cm, Cin, ct.c_void_p(out.ctypes.data)))
    want = WP.pair_taps_f32(g, S)
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(out[:, :, :Cm], W.taps_f32(g))
    assert np.array_equal(out[0, :, Cm:], S[:, :Cin // 2]) and np.array_equal(out[3, :, Cm:], -S[:, :Cin // 2])
    assert np.array_equal(out[1, :, Cm:] * np.float32(2), S[:, Cin // 2:]) and np.array_equal(out[1, :, Cm:], out[2, :, Cm:])
