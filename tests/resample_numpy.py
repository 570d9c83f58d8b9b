"""float64 restatements of torchaudio.transforms.Resample(orig, new, "sinc_interp_hann", lowpass_filter_width, rolloff) for the resampler's
tests (no torch, no library code):
  closed_form   out[m] = sum_n x[n] g(n / O - m / N) straight from the definition, the contract of lds_resample (include/lds.h);
  conv_form     torchaudio's two functions, _get_sinc_resample_kernel + _apply_sinc_resample_kernel, restated line by line: the
                N x (2 width + O) bank, the (width, width + O) padding, the stride-O convolution and the crop to ceil(N L / O);
  apply_bank64  a given fp32 bank (the library's) applied in float64, with sum |x| |g| for the a-priori rounding bound."""
import math

import numpy as np


def reduced(orig, new):
    g = math.gcd(int(orig), int(new))
    return int(orig) // g, int(new) // g


def out_length(L, O, N):
    return -((-int(L) * N) // O)


def g_of(d, O, N, w=6, rolloff=0.99):
    """the filter at the integer offset d = n N - m O, i.e. at tau = d / (O N): (B / O) sinc(u) cos^2(pi u / (2 w)), u = clamp(B tau, -w, w)"""
    base = rolloff * min(O, N)
    u = np.clip(base * np.asarray(d, dtype=np.float64) / (O * N), -float(w), float(w))
    return (base / O) * np.sinc(u) * np.cos(np.pi * u / (2.0 * w)) ** 2


def support_half(O, N, w=6, rolloff=0.99):
    """the filter is at its clamp (below 1e-30) for |d| >= this"""
    return w * O * N / (rolloff * min(O, N))


def closed_form(x, orig, new, w=6, rolloff=0.99):
    x = np.asarray(x, dtype=np.float64)
    O, N = reduced(orig, new)
    L, half = len(x), support_half(O, N, w, rolloff)
    out = np.zeros(out_length(L, O, N))
    for m in range(len(out)):
        lo = max(0, int(math.floor((m * O - half) / N)) - 1)            # a sample or two more than the support: g is at its clamp there
        hi = min(L - 1, int(math.ceil((m * O + half) / N)) + 1)
        n = np.arange(lo, hi + 1, dtype=np.int64)
        out[m] = np.dot(x[lo:hi + 1], g_of(n * N - m * O, O, N, w, rolloff))
    return out


def conv_kernel(O, N, w=6, rolloff=0.99, rows=None, cols=None):
    """_get_sinc_resample_kernel: [N][2 width + O] (or the given rows / columns of it), and width.  The filter argument
    t = (-i / N + idx / O) base_freq is formed in extended precision (`real`) and rounded to float64 once: in float64 the two fractions
    cancel and base_freq multiplies what is left of their rounding, 2^-53 x 2 x 15,840 = 3.5e-12 in t at 16000 -> 16001 -- the
    formulation's own error, which would otherwise be what a comparison at 1e-12 measures (3.4e-12 there at 5000 samples of N(0, 1))."""
    real = np.longdouble
    base_freq = min(O, N) * rolloff
    width = math.ceil(w * O / base_freq)
    idx = np.arange(-width, width + O, dtype=real)[None, :] / O
    ph = np.arange(0, -N, -1, dtype=real)[:, None] / N
    if rows is not None:
        ph = ph[rows]
    if cols is not None:
        idx = idx[:, cols]
    t = ph + idx
    t *= real(base_freq)
    t = np.clip(t, -w, w).astype(np.float64)
    window = np.cos(t * math.pi / w / 2) ** 2
    t *= math.pi
    scale = base_freq / O
    with np.errstate(invalid="ignore", divide="ignore"):
        kernels = np.where(t == 0, 1.0, np.sin(t) / t)
    kernels *= window * scale
    return kernels, width


def conv_form(x, orig, new, w=6, rolloff=0.99):
    """_apply_sinc_resample_kernel: pad (width, width + O), convolve with stride O, interleave the N phases, crop.  The bank is formed in
    blocks of phases, and only in the columns that meet a sample of x in some window (the others multiply the zero padding): 16000 -> 16001
    has 16,001 x 16,014 entries."""
    x = np.asarray(x, dtype=np.float64)
    O, N = reduced(orig, new)
    L = len(x)
    width = math.ceil(w * O / (min(O, N) * rolloff))
    K = 2 * width + O
    xp = np.concatenate([np.zeros(width), x, np.zeros(width + O)])
    Q = (len(xp) - K) // O + 1
    win = np.lib.stride_tricks.sliding_window_view(xp, K)[::O][:Q]      # [Q][K]
    pos = np.arange(Q)[:, None] * O + np.arange(K)[None, :] - width      # the sample each entry of a window holds
    cols = np.nonzero(((pos >= 0) & (pos < L)).any(axis=0))[0]
    out = np.zeros((Q, N))
    M = out_length(L, O, N)
    for r0 in range(0, N if Q > 1 else min(N, M), 1024):      # (one window: the phases beyond the crop are never looked at)
        rows = slice(r0, min(N, r0 + 1024))
        out[:, rows] = win[:, cols] @ conv_kernel(O, N, w, rolloff, rows, cols)[0].T
    return out.reshape(-1)[:M]


def apply_bank64(x, O, N, bankT, first, length=None, chunk=1 << 16):
    """sum_k x[(m / N) O + first[m % N] + k] bankT[k][m % N] in float64 for m < ceil(N length / O), x zero outside [0, length); returns
    (out, bound): bound[m] = gamma(taps of m's phase + 1) sum |x| |g|, the a-priori rounding bound of the fp32 chain.  A phase's taps are its
    non-zero bank entries (a zero entry adds no rounding error: fmaf(x, 0, acc) = acc)."""
    x = np.asarray(x, dtype=np.float64)
    length = len(x) if length is None else int(length)
    T = bankT.shape[0]
    b64 = np.asarray(bankT, dtype=np.float64)
    M = out_length(length, O, N)
    out, bound = np.zeros(M), np.zeros(M)
    gam = gamma((b64 != 0).sum(axis=0) + 1)
    xz = np.concatenate([x[:length], [0.0]])      # index `length` = the zero outside the clip
    k = np.arange(T, dtype=np.int64)[None, :]
    for m0 in range(0, M, chunk):
        m = np.arange(m0, min(M, m0 + chunk), dtype=np.int64)
        i = m % N
        n = ((m // N) * O + first[i].astype(np.int64))[:, None] + k
        v = xz[np.where((n >= 0) & (n < length), n, length)]
        g = b64[:, i].T
        out[m0:m0 + len(m)] = (v * g).sum(axis=1)
        bound[m0:m0 + len(m)] = gam[i] * (np.abs(v) * np.abs(g)).sum(axis=1)
    return out, bound


def gamma(T):
    """the a-priori constant of an fp32 dot product (any summation order, with or without FMA) with T = its terms + 1:
    T u / (1 - T u), u = 2^-24"""
    u, T = 2.0 ** -24, np.asarray(T, dtype=np.float64)
    return T * u / (1.0 - T * u)
