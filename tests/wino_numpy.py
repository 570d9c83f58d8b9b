"""Specification of the Winograd F(2,3) form of the resnets' k 3 / stride 1 / pad 1 convolution (csrc/conv_wino.hip), restated in numpy.

With g the three taps and d the padded input -- d[n] = x[n - 1], zero outside frames 0 .. T-1 of x -- the convolution is
Y[t] = g0 d[t] + g1 d[t+1] + g2 d[t+2], and per output pair i (P = ceil(T / 2) pairs):
    U0 = g0, U1 = (g0 + g1 + g2) / 2, U2 = (g0 - g1 + g2) / 2, U3 = g2                                  (weights, once)
    V0 = d[2i] - d[2i+2], V1 = d[2i+1] + d[2i+2], V2 = d[2i+2] - d[2i+1], V3 = d[2i+1] - d[2i+3]        (inputs)
    Mj = Uj . Vj (sum over the input channels);   Y[2i] = M0 + M1 + M2,   Y[2i+1] = M1 - M2 - M3
A frame at or beyond an utterance's length is zero in x whatever the tensor holds there; with an odd T the last pair's second output
does not exist and its d[2i+3] is zero.

level_len / gn_act / ragged_reference restate what surrounds the convolution in a resnet (run_resnet: the lengths at a level, GroupNorm with
scale / shift and SiLU, bias, residual) for the kernel tests of tests/test_gpu_wino_modes.py, every utterance alone in float64."""
import numpy as np


def taps(g):
    """g [Co, Ci, 3] -> U [4, Co, Ci] in float64"""
    g = np.asarray(g, dtype=np.float64)
    g0, g1, g2 = g[..., 0], g[..., 1], g[..., 2]
    return np.stack([g0, (g0 + g1 + g2) * 0.5, (g0 - g1 + g2) * 0.5, g2])


def taps_f32(g):
    """the float64 transform rounded once to fp32: what lds_test_wino_pack returns"""
    return taps(g).astype(np.float32)


def padded(x, length=None):
    """x [..., T] -> d [..., 2 P + 2] with d[n] = x[n - 1], zero outside 0 <= n - 1 < min(T, length): garbage beyond a length (NaN, Inf)
    is replaced, not multiplied"""
    x = np.asarray(x)
    T = x.shape[-1]
    P = (T + 1) // 2
    L = T if length is None else min(int(length), T)
    d = np.zeros(x.shape[:-1] + (2 * P + 2,), dtype=x.dtype)
    d[..., 1:L + 1] = x[..., :L]
    return d


def planes(x, length=None):
    """x [C, T] -> V [4, C, P] in x's dtype"""
    d = padded(x, length)
    P = (x.shape[-1] + 1) // 2
    i = 2 * np.arange(P)
    return np.stack([d[..., i] - d[..., i + 2], d[..., i + 1] + d[..., i + 2], d[..., i + 2] - d[..., i + 1], d[..., i + 1] - d[..., i + 3]])


def conv(x, g, length=None):
    """x [Ci, T], g [Co, Ci, 3] -> Y [Co, T] through F(2,3), in float64; frames at and beyond `length` are zero in the input and the output"""
    x = np.asarray(x, dtype=np.float64)
    T = x.shape[-1]
    U, V = taps(g), planes(x, length)
    M = np.einsum("joc,jcp->jop", U, V)
    Y = np.empty((g.shape[0], 2 * V.shape[-1]))
    Y[:, 0::2] = M[0] + M[1] + M[2]
    Y[:, 1::2] = M[1] - M[2] - M[3]
    Y = Y[:, :T]
    if length is not None:
        Y[:, int(length):] = 0.0
    return Y


def direct(x, g, length=None):
    """the k 3 / pad 1 convolution as a plain sum, float64"""
    x = np.asarray(x, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64)
    T = x.shape[-1]
    L = T if length is None else min(int(length), T)
    xp = np.zeros((x.shape[0], T + 2))
    xp[:, 1:L + 1] = x[:, :L]
    Y = sum(g[:, :, k] @ xp[:, k:k + T] for k in range(3))
    Y[:, L:] = 0.0
    return Y


def level_len(n, lvl):
    """a level-0 length at level lvl of the UNet, as the kernels reduce it: (n - 1) / 2 + 1 per level (the k 3 / stride 2 / pad 1 downsampler's
    output length, ceil(n / 2))"""
    n = int(n)
    for _ in range(int(lvl)):
        n = (n - 1) // 2 + 1
    return n


def silu(x):
    return x / (1.0 + np.exp(-x))


def gn_act(x, gamma, beta, groups, scale=None, shift=None, act=True, eps=1e-5):
    """x [C, L] (one utterance, its own frames only) -> act(GroupNorm(x) (* (1 + scale) + shift)) in float64"""
    x = np.asarray(x, dtype=np.float64)
    C, L = x.shape
    xg = x.reshape(groups, -1)
    xn = ((xg - xg.mean(1, keepdims=True)) / np.sqrt(xg.var(1, keepdims=True) + eps)).reshape(C, L)
    xn = xn * np.asarray(gamma, dtype=np.float64)[:, None] + np.asarray(beta, dtype=np.float64)[:, None]
    if scale is not None:
        xn = xn * (1.0 + np.asarray(scale, dtype=np.float64)[:, None]) + np.asarray(shift, dtype=np.float64)[:, None]
    return silu(xn) if act else xn


def ragged_reference(x, lengths, lvl, gamma, beta, groups, g, bias=None, scale_shift=None, res=None, act=True):
    """The routed resnet convolution on a ragged batch at level lvl, every utterance ALONE and cut to its reduced length, in float64:
    x [B, Ci, T] (the tensor at level lvl; whatever it holds at and beyond a reduced length is never read), lengths = LEVEL-0 lengths (None:
    every utterance has T frames), scale_shift [B, 2 Ci] (scales, then shifts) or None, res [B, Co, T] or None.
    -> (d [B, Ci, T], Y [B, Co, T], L [B]): the activated GroupNorm output, the convolution (+ bias, + res) -- both zero from the reduced
    length on -- and the reduced lengths"""
    x = np.asarray(x)
    B, Ci, T = x.shape
    Co = g.shape[0]
    L = [T if lengths is None else level_len(lengths[b], lvl) for b in range(B)]
    d, Y = np.zeros((B, Ci, T)), np.zeros((B, Co, T))
    for b in range(B):
        n = L[b]
        assert 1 <= n <= T, (b, n, T)
        sc, sh = (None, None) if scale_shift is None else (scale_shift[b, :Ci], scale_shift[b, Ci:])
        d[b, :, :n] = gn_act(x[b, :, :n], gamma, beta, groups, sc, sh, act)
        y = direct(d[b, :, :n], g)
        if bias is not None:
            y = y + np.asarray(bias, dtype=np.float64)[:, None]
        if res is not None:
            y = y + np.asarray(res[b, :, :n], dtype=np.float64)
        Y[b, :, :n] = y
    return d, Y, L


def planes_device_layout(V):
    """V [B, 4, C, P] -> the device's plane tensor [B][C/8][2][4][P][4] (channel 8q + 2j + h at element j of row (q, h), as K4P)"""
    B, _, C, P = V.shape
    return np.ascontiguousarray(V.reshape(B, 4, C // 8, 4, 2, P).transpose(0, 2, 4, 1, 5, 3))
