"""Winograd F(2,3) for the resnets' k 3 convolutions (csrc/conv_wino.hip), the parts that need no GPU: the restatement of
tests/wino_numpy.py against the direct convolution in float64, its zero rules for odd lengths and ragged utterances, and the host-side
weight transform of the library (lds_test_wino_pack) against the float64 transform rounded once; the level reduction of lengths and the
ragged per-utterance reference that tests/test_gpu_wino_modes.py compares the kernels with."""
import ctypes as ct

import numpy as np
import pytest

import wino_numpy as W


def U(name, shape, lo=-1.0, hi=1.0):
    from lds import init_weights
    return init_weights.uniform("wino.cpu." + name, shape, 26, lo, hi)


@pytest.mark.parametrize("T", [1, 2, 3, 5, 64, 65])
def test_f23_equals_direct_float64(T):
    Ci, Co = 24, 16
    x = U(f"x{T}", (Ci, T), -2, 2).astype(np.float64)
    g = U(f"g{T}", (Co, Ci, 3)).astype(np.float64) / np.sqrt(3 * Ci)
    got, ref = W.conv(x, g), W.direct(x, g)
    assert got.shape == ref.shape == (Co, T)
    assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("T", [1, 3, 5, 65])
def test_odd_length_zero_rule(T):
    """the last odd frame's partner and its d[2i+3] are zero: the last pair's planes are those of the input extended by zeros"""
    x = U(f"odd{T}", (8, T), -2, 2)
    V = W.planes(x)
    P = (T + 1) // 2
    assert V.shape == (4, 8, P)
    last, before = x[:, T - 1], (x[:, T - 2] if T > 1 else np.zeros(8, dtype=x.dtype))
    # pair P-1 of an odd T: d[2i] = x[T-2], d[2i+1] = x[T-1], d[2i+2] = d[2i+3] = 0
    assert np.array_equal(V[0, :, P - 1], before) and np.array_equal(V[1, :, P - 1], last)
    assert np.array_equal(V[2, :, P - 1], -last) and np.array_equal(V[3, :, P - 1], last)
    # pair 0 starts at the left pad frame: d[0] = 0
    ext = np.concatenate([x, np.zeros((8, 3), dtype=x.dtype)], axis=1)
    assert np.array_equal(V[0, :, 0], -ext[:, 1])


@pytest.mark.parametrize("T,length", [(130, 37), (130, 130), (64, 1), (65, 64), (6, 3)])
def test_ragged_zero_rule(T, length):
    """frames at and beyond an utterance's length are zero in d whatever the tensor holds there: NaN / Inf never reach a plane, and the
    result equals the utterance convolved alone"""
    Ci, Co = 16, 16
    x = U(f"rg{T}.{length}", (Ci, T), -2, 2)
    g = U(f"rgw{T}.{length}", (Co, Ci, 3)) / np.float32(np.sqrt(3 * Ci))
    bad = x.copy()
    bad[:, length:] = np.where(np.arange(T - length) % 2 == 0, np.nan, np.inf)
    V = W.planes(bad, length)
    assert np.isfinite(V).all()
    assert np.array_equal(V[:, :, :(length + 1) // 2], W.planes(x[:, :length]))
    assert not V[:, :, (length + 2) // 2:].any()      # pairs wholly beyond the length (and one frame of margin) are zero
    got = W.conv(bad, g, length)
    alone = W.direct(x[:, :length].astype(np.float64), g)
    assert np.isfinite(got).all()
    assert np.abs(got[:, :length] - alone).max() <= 1e-12 * max(1.0, np.abs(alone).max())
    assert not got[:, length:].any()


def test_level_len_is_repeated_ceil_halving():
    """the kernels' (n - 1) / 2 + 1 per level against ceil(n / 2) applied lvl times, and against ceil(n / 2^lvl) outright"""
    import math
    for n in list(range(1, 1100)) + [2047, 2048, 2049, 4097, 2 ** 20 + 1]:
        want = n
        for lvl in range(6):
            assert W.level_len(n, lvl) == want == -(-n // 2 ** lvl), (n, lvl)
            want = math.ceil(want / 2)
    assert [W.level_len(n, 2) for n in (520, 37, 259)] == [130, 10, 65]
    assert [W.level_len(n, 3) for n in (130, 37, 1, 129)] == [17, 5, 1, 17]


@pytest.mark.parametrize("lvl,T,lengths", [(0, 70, [70, 33, 1]), (1, 65, [130, 37, 1, 129]), (2, 130, [520, 37, 259]), (3, 17, [130, 37, 1, 129])])
def test_ragged_reference_at_a_level(lvl, T, lengths):
    """every utterance equals its own cut tensor run alone as a dense batch of one; whatever the tensor holds beyond a reduced length
    (NaN, Inf) changes nothing; zeros beyond; the normalised tensor has the group statistics GroupNorm promises"""
    B, Ci, Co, groups = len(lengths), 32, 16, 2
    tag = f"lv{lvl}.{T}"
    x, res = U(tag + ".x", (B, Ci, T), -2, 2) + np.float32(0.3), U(tag + ".res", (B, Co, T))
    gamma, beta, ss = U(tag + ".g", (Ci,), 0.5, 1.5), U(tag + ".b", (Ci,), -0.5, 0.5), U(tag + ".ss", (B, 2 * Ci), -0.5, 0.5)
    g, bias = U(tag + ".w", (Co, Ci, 3)) / np.float32(np.sqrt(3 * Ci)), U(tag + ".bias", (Co,))
    d, Y, L = W.ragged_reference(x, lengths, lvl, gamma, beta, groups, g, bias, ss, res)
    assert L == [-(-n // 2 ** lvl) for n in lengths] and d.dtype == Y.dtype == np.float64
    bad = x.copy()
    for b, n in enumerate(L):
        bad[b, :, n:] = np.nan
        bad[b, :, n + 1:] = np.inf
    d2, Y2, _ = W.ragged_reference(bad, lengths, lvl, gamma, beta, groups, g, bias, ss, res)
    assert np.array_equal(d, d2) and np.array_equal(Y, Y2)
    for b, n in enumerate(L):
        assert not d[b, :, n:].any() and not Y[b, :, n:].any()
        da, Ya, La = W.ragged_reference(x[b:b + 1, :, :n], None, 0, gamma, beta, groups, g, bias, ss[b:b + 1], res[b:b + 1, :, :n])
        assert La == [n] and np.array_equal(da[0], d[b, :, :n]) and np.array_equal(Ya[0], Y[b, :, :n])
        # the convolution of the reference is the F(2,3) form of the same tensor
        assert np.abs(W.conv(d[b], g, n)[:, :n] + bias[:, None] + res[b, :, :n] - Y[b, :, :n]).max() < 1e-12
        plain = W.gn_act(x[b, :, :n], np.ones(Ci), np.zeros(Ci), groups, act=False).reshape(groups, -1)
        assert np.abs(plain.mean(1)).max() < 1e-12
        assert np.abs(plain.var(1) - 1.0).max() < 1e-3      # (var / (var + eps), 16 channels x n frames per group)


def test_device_plane_layout_roundtrip():
    V = np.arange(2 * 4 * 16 * 3, dtype=np.float32).reshape(2, 4, 16, 3)
    D = W.planes_device_layout(V)
    assert D.shape == (2, 2, 2, 4, 3, 4)
    for c in (0, 1, 6, 9, 15):
        q, e, h = c // 8, (c % 8) // 2, c % 2
        assert np.array_equal(D[:, q, h, :, :, e], V[:, :, c, :])


@pytest.mark.parametrize("Co,Ci", [(1, 1), (16, 24), (96, 32)])
def test_pack_matches_float64_transform(Co, Ci):
    from lds import native
    g = U(f"pack{Co}.{Ci}", (Co, Ci, 3), -3, 3)
    g[0, 0] = [1.0, 2.0 ** -24, -1.0]      # g0 + g1 + g2 is not representable in fp32: a transform in fp32 would round twice
    out = np.full((4, Co, Ci), np.nan, dtype=np.float32)
    native.check(native.lib().lds_test_wino_pack(ct.c_void_p(g.ctypes.data), Co, Ci, ct.c_void_p(out.ctypes.data)))
    want = W.taps_f32(g)
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    assert out[1, 0, 0] == np.float32(2.0 ** -25) and out[2, 0, 0] == np.float32(-(2.0 ** -25))
