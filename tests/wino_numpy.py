"""Specification of the Winograd F(2,3) form of the resnets' k 3 / stride 1 / pad 1 convolution (csrc/conv_wino.hip), restated in numpy.

With g the three taps and d the padded input -- d[n] = x[n - 1], zero outside frames 0 .. T-1 of x -- the convolution is
Y[t] = g0 d[t] + g1 d[t+1] + g2 d[t+2], and per output pair i (P = ceil(T / 2) pairs):
    U0 = g0, U1 = (g0 + g1 + g2) / 2, U2 = (g0 - g1 + g2) / 2, U3 = g2                                  (weights, once)
    V0 = d[2i] - d[2i+2], V1 = d[2i+1] + d[2i+2], V2 = d[2i+2] - d[2i+1], V3 = d[2i+1] - d[2i+3]        (inputs)
    Mj = Uj . Vj (sum over the input channels);   Y[2i] = M0 + M1 + M2,   Y[2i+1] = M1 - M2 - M3
A frame at or beyond an utterance's length is zero in x whatever the tensor holds there; with an odd T the last pair's second output
does not exist and its d[2i+3] is zero."""
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


def planes_device_layout(V):
    """V [B, 4, C, P] -> the device's plane tensor [B][C/8][2][4][P][4] (channel 8q + 2j + h at element j of row (q, h), as K4P)"""
    B, _, C, P = V.shape
    return np.ascontiguousarray(V.reshape(B, 4, C // 8, 4, 2, P).transpose(0, 2, 4, 1, 5, 3))
