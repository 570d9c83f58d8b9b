"""Specification of a resnet's conv2 + 1x1 shortcut as ONE Winograd F(2,3) reduction (csrc/model.hip wino_pair_taps / run_wconv_pair, DESIGN.md
41), restated in numpy on top of tests/wino_numpy.py.

conv_wino joins Y[2i] = M0 + M1 + M2 and Y[2i+1] = M1 - M2 - M3.  An addend on M0 reaches the even frame only, one on M3 the odd frame only
(negated), and a pair (A on M1, B on M2) puts A + B into the even and A - B into the odd frame.  With x = [x1 ; x2] the raw block input,
x_e[i] = x[2i], x_o[i] = x[2i+1] (zero from the utterance's length on), S the shortcut's [Co, Cin] matrix and x's channels split into a first
half A and a second half B, the reduction is extended by Cin / 2 channels:
    tap 0: S_A . x_e(A)      tap 1: S_B / 2 . (x_e(B) + x_o(B))      tap 2: S_B / 2 . (x_e(B) - x_o(B))      tap 3: -S_A . x_o(A)
so that every one of the four products is Cm + Cin / 2 deep: 2 Cm + Cin column-products per output pair where the direct form has 3 Cm + Cin.
Halving S_B is exact in fp32; the two plane operations are one fp32 addition each."""
import numpy as np

import wino_numpy as W


def pair_taps(g, S):
    """g [Co, Cm, 3], S [Co, Cin] -> U [4, Co, Cm + Cin/2] in float64"""
    S = np.asarray(S, dtype=np.float64)
    half = S.shape[1] // 2
    sa, sb = S[:, :half], S[:, half:]
    return np.concatenate([W.taps(g), np.stack([sa, sb * 0.5, sb * 0.5, -sa])], axis=2)


def pair_taps_f32(g, S):
    """the float64 transform rounded once to fp32: what lds_test_wino_pair_pack returns"""
    return pair_taps(g, S).astype(np.float32)


def side_planes(x, length=None):
    """x [Cin, T] (raw block input) -> [4, Cin/2, P] in x's dtype: x_e(A), x_e(B) + x_o(B), x_e(B) - x_o(B), x_o(A); whatever x holds at and
    beyond `length` is replaced by zero, not multiplied"""
    x = np.asarray(x)
    Cin, T = x.shape
    P = (T + 1) // 2
    L = T if length is None else min(int(length), T)
    z = np.zeros((Cin, 2 * P), dtype=x.dtype)
    z[:, :L] = x[:, :L]
    xe, xo = z[:, 0::2], z[:, 1::2]
    half = Cin // 2
    return np.stack([xe[:half], xe[half:] + xo[half:], xe[half:] - xo[half:], xo[:half]])


def pair_planes(d, x, length=None):
    """d [Cm, T] (conv2's activated input), x [Cin, T] -> V [4, Cm + Cin/2, P]"""
    return np.concatenate([W.planes(d, length), side_planes(x, length)], axis=1)


def pair_conv(d, x, g, S, length=None):
    """conv_k3(d; g) + S x through the extended F(2,3) form, float64 -> [Co, T], zero from `length` on"""
    d, x = np.asarray(d, dtype=np.float64), np.asarray(x, dtype=np.float64)
    T = d.shape[-1]
    U, V = pair_taps(g, S), pair_planes(d, x, length)
    M = np.einsum("joc,jcp->jop", U, V)
    Y = np.empty((U.shape[1], 2 * V.shape[-1]))
    Y[:, 0::2] = M[0] + M[1] + M[2]
    Y[:, 1::2] = M[1] - M[2] - M[3]
    Y = Y[:, :T]
    if length is not None:
        Y[:, int(length):] = 0.0
    return Y


def pair_direct(d, x, g, S, length=None):
    """the same as plain sums, float64"""
    x = np.asarray(x, dtype=np.float64)
    T = x.shape[-1]
    L = T if length is None else min(int(length), T)
    Y = W.direct(d, g, length)
    Y[:, :L] += np.asarray(S, dtype=np.float64) @ x[:, :L]
    return Y
