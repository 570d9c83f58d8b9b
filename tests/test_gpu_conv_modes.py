"""conv_dma / conv_bf3 modes that the product reaches through whole models only, each against a float64 numpy reference through a
single-op entry of include/lds_test.h:

  lds_test_dconv_pair   the fused resnet tail (conv2 k 3 + 1x1 shortcut over [x1 ; x2] + GroupNorm partials; tile variants, cluster split-K)
  lds_test_dconv_ex     EPI_GELU with the encoders' geometries, per-utterance lengths inside a convolution, GroupNorm partials from k 3 tiles
  lds_test_voc_ups      the vocoder's polyphase ConvTranspose on conv_dma with the raw + LeakyReLU store and per-utterance lengths

Tolerance: max|got - ref| < EPS * max|ref| with EPS = 2e-5, the bound test_conv_dma / test_conv_bf3 hold these kernels to, in all three
formats.  GroupNorm partials: the output bound propagated (mean within EPS * A; M2 within 2 EPS A sum|y - mean| + n (EPS A)^2, A = max|ref|).
A ragged case's reference is every utterance cut to its own length and computed alone.  Results are computed once per (case, format) and
shared by the test functions of a group; the last function of a group asserts that the launch configurations cover the variants."""
import ctypes as ct
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EPS = 2e-5
FMT = {"f32": -1, "bf16x3": 0, "f16x2": 1}


def U(name, shape, lo=-1.0, hi=1.0):
    from lds import init_weights
    return init_weights.uniform("cm." + name, shape, 11, lo, hi)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def host(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def P(a):
    return ct.c_void_p(a.ctypes.data) if a is not None else None


def D(t):
    return ct.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def nan_out(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def i32(v):
    return None if v is None else np.ascontiguousarray(v, dtype=np.int32)


# ---- float64 references ---------------------------------------------------------------------------------------------------------
def conv64(x, w, bias=None, stride=1, pad=0):
    """Conv1d by its definition: x [B][Ci][T], w [Co][Ci][K] -> [B][Co][(T + 2 pad - K) / stride + 1]"""
    x, w = x.astype(np.float64), w.astype(np.float64)
    K = w.shape[2]
    To = (x.shape[2] + 2 * pad - K) // stride + 1
    xp = np.pad(x, ((0, 0), (0, 0), (pad, pad)))
    y = np.zeros((x.shape[0], w.shape[0], To))
    for k in range(K):
        y += np.einsum("oc,bct->bot", w[:, :, k], xp[:, :, k:k + (To - 1) * stride + 1:stride])
    if bias is not None:
        y += bias.astype(np.float64)[None, :, None]
    return y


def gelu64(v):
    from scipy.special import erf
    return 0.5 * v * (1.0 + erf(v / np.sqrt(2.0)))


def lrelu64(v, slope=0.1):
    return np.where(v >= 0, v, v * slope)


def epilogue64(y, gelu, res):
    """csrc/kernels.h EPI_GELU: GELU of the biased / normalised value, before the residual"""
    if gelu:
        y = gelu64(y)
    if res is not None:
        y = y + res.astype(np.float64)
    return y


def layer_norm64(x, gamma, beta, eps):
    x = x.astype(np.float64)
    mu = x.mean(1, keepdims=True)
    var = ((x - mu) ** 2).mean(1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * gamma.astype(np.float64)[None, :, None] + beta.astype(np.float64)[None, :, None]


def conv_transpose64(x, w, bias, stride, pad):
    """ConvTranspose1d by its definition: y[b, co, t * stride + k - pad] += x[b, ci, t] * w[ci, co, k]"""
    x, w = x.astype(np.float64), w.astype(np.float64)
    B, _, T = x.shape
    Co, K = w.shape[1], w.shape[2]
    full = np.zeros((B, Co, (T - 1) * stride + K))
    for k in range(K):
        full[:, :, k:k + (T - 1) * stride + 1:stride] += np.einsum("bct,co->bot", x, w[:, :, k])
    y = full[:, :, pad:full.shape[2] - pad]
    if bias is not None:
        y = y + bias.astype(np.float64)[None, :, None]
    return y


def lvl_len(n, lvl):
    """csrc/k4p.h ragged_len: a level halves a length the way the stride-2 convolutions do"""
    for _ in range(lvl):
        n = (n - 1) // 2 + 1
    return n


def valid_len(n, lvl, T):
    return min(lvl_len(int(n), lvl), T)


def cut(x, n):
    """the tensor of a ragged batch: zeros at and beyond every utterance's length"""
    if x is None:
        return None
    x = x.copy()
    for b, nb in enumerate(n):
        x[b, :, nb:] = 0
    return x


def alone(fn, n_in, n_out, To, *tensors):
    """the ragged reference: fn on every utterance cut to its own n_in[b] frames, alone; zeros from its n_out[b] output frames on"""
    rows = []
    for b in range(len(n_in)):
        y = fn(*[None if t is None else t[b:b + 1, :, :n_in[b]] for t in tensors], b)
        assert y.shape[2] == n_out[b], (y.shape, n_out[b])      # (the lengths the test hands the kernel are the reference's own)
        rows.append(np.pad(y, ((0, 0), (0, 0), (0, To - n_out[b]))))
    return np.concatenate(rows, 0)


# ---- the shared checks ------------------------------------------------------------------------------------------------------------
def err_over_scale(got, ref):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all()
    return float(np.abs(got.astype(np.float64) - ref).max() / np.abs(ref).max())


def gn_partial_errors(gn, ref, n_out):
    """(mean error / A, EPS * worst M2 error / its bound) over the (16 channels x 32 frames) blocks with at least one valid frame"""
    B, Co, To = ref.shape
    A = np.abs(ref).max()
    assert gn.shape == (B, Co // 16, (To + 31) // 32, 2)
    e_mean, e_m2 = 0.0, 0.0
    for b in range(B):
        for tb in range((n_out[b] + 31) // 32):
            blk = ref[b, :, tb * 32:min(tb * 32 + 32, n_out[b])].reshape(Co // 16, -1)
            mean = blk.mean(1)
            dev_ = np.abs(blk - mean[:, None])
            m2 = (dev_ ** 2).sum(1)
            bound = 2 * EPS * A * dev_.sum(1) + blk.shape[1] * (EPS * A) ** 2
            g = gn[b, :, tb].astype(np.float64)
            assert np.isfinite(g).all(), (b, tb)
            e_mean = max(e_mean, float(np.abs(g[:, 0] - mean).max() / A))
            e_m2 = max(e_m2, float(EPS * (np.abs(g[:, 1] - m2) / bound).max()))
    return e_mean, e_m2


def assert_zero_tail(out, n_out):
    for b, nb in enumerate(n_out):
        assert (out[b, :, nb:] == 0).all(), f"utterance {b}: a non-zero (or NaN) frame at or beyond its length {nb}"


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ==================================================================================================================================
# the fused resnet tail
# ==================================================================================================================================
# name: (B, Cm, Co, C1, C2, T, lengths (level 0) or None, lvl, tile_batch, the fp32 launch's "BM<bm> ... BK32+<bk1>" by conv_dma.hip dma_pick /
# pair_variant).  BM 32: fewer 64 x 64 tiles than CUs at the nominal batch of 16 (Mp / 64 * ceil(T / 64) * 16 <= 256, or < 512 and not a
# multiple of 256); BM 64: more, with Mp no multiple of 128 (no 128 x 128 candidate).  BK1 64: C1 and C1 + C2 multiples of 64.
PAIR = {
    "x2_bm32_bk64_t37": (2, 64, 128, 128, 128, 37, None, 0, 0, (32, 64)),
    "x2_bm32_bk32_t64": (2, 96, 64, 64, 96, 64, None, 0, 0, (32, 32)),
    "x1_bm32_bk64_t65": (2, 128, 192, 128, 0, 65, None, 0, 0, (32, 64)),
    "x1_bm32_bk32_t130": (1, 64, 128, 96, 0, 130, None, 0, 0, (32, 32)),
    "x2_bm64_bk64_t130": (1, 64, 704, 64, 64, 130, None, 0, 0, (64, 64)),
    "x1_bm64_bk32_t130": (2, 32, 704, 96, 0, 130, None, 0, 0, (64, 32)),
    "x2_bm64_bk32_t65": (1, 64, 1088, 64, 96, 65, None, 0, 0, (64, 32)),
    "x2_bm64_bk32_t37": (1, 32, 2112, 32, 32, 37, None, 0, 0, (64, 32)),
    "x1_bm64_bk64_t64": (1, 32, 2112, 64, 0, 64, None, 0, 0, (64, 64)),
    "ragged_lvl0": (4, 64, 128, 64, 64, 130, [130, 65, 33, 1], 0, 0, (32, 64)),
    "ragged_lvl1": (4, 64, 128, 64, 64, 65, [130, 129, 66, 2], 1, 0, (32, 64)),      # (n - 1) / 2 + 1: 65, 65, 33, 1
    "ragged_bm64": (3, 32, 704, 64, 32, 130, [130, 97, 64], 0, 0, (64, 32)),
    "full_lvl0": (4, 64, 128, 64, 64, 130, [130, 130, 130, 130], 0, 0, (32, 64)),    # == dense_twin bit for bit
    "dense_twin": (4, 64, 128, 64, 64, 130, None, 0, 0, (32, 64)),
    "b1_ks4": (1, 128, 128, 128, 128, 64, None, 0, 1, (32, 64)),                      # 4 tiles, 4 + 4 K-steps: four workgroups per tile
    "b2_ks2": (2, 128, 192, 128, 0, 130, None, 0, 2, (32, 64)),                       # 36 tiles, 4 + 2 K-steps: two
    "b2_ks1": (2, 64, 64, 64, 96, 37, None, 0, 2, (32, 32)),                          # 2 + 5 K-steps: no split
}
PAIR_IDS = [(n, f) for n in PAIR for f in FMT]


def pair_id(n, f):
    return f"{n}-{f}" + ("-lat" if PAIR[n][8] else "")


_pair_ref, _pair_run = {}, {}


def pair_inputs(name):
    """inputs and float64 reference of a case: one per case, shared by the three formats"""
    if name in _pair_ref:
        return _pair_ref[name]
    B, Cm, Co, C1, C2, T, lengths, lvl, _, _ = PAIR[name]
    key = f"pair.{Cm}.{Co}.{C1}.{C2}.{T}"
    h, x1 = U(key + ".h", (B, Cm, T), -2, 2), U(key + ".x1", (B, C1, T), -2, 2)
    x2 = U(key + ".x2", (B, C2, T), -2, 2) if C2 else None
    w3 = U(key + ".w3", (Co, Cm, 3)) / np.float32(np.sqrt(Cm * 3))
    w1 = U(key + ".w1", (Co, C1 + C2, 1)) / np.float32(np.sqrt(C1 + C2))
    b3, b1 = U(key + ".b3", (Co,), 0.5, 1.5), U(key + ".b1", (Co,), -0.25, 0.25)      # a non-zero sum: an unmasked store shows
    n = [valid_len(v, lvl, T) for v in lengths] if lengths else [T] * B
    h, x1, x2 = cut(h, n), cut(x1, n), cut(x2, n)

    def one(hh, xa, xb, b):
        x = xa if xb is None else np.concatenate([xa, xb], 1)
        return conv64(hh, w3, b3, pad=1) + conv64(x, w1, b1)
    ref = alone(one, n, n, T, h, x1, x2)
    _pair_ref[name] = dict(h=h, x1=x1, x2=x2, w3=host(w3), w1=host(w1), b3=host(b3), b1=host(b1), n=n, ref=ref)
    return _pair_ref[name]


def pair_result(name, fmt):
    if (name, fmt) in _pair_run:
        return _pair_run[name, fmt]
    from lds import native
    B, Cm, Co, C1, C2, T, lengths, lvl, tile_batch, _ = PAIR[name]
    i = pair_inputs(name)
    dh, d1, d2 = dev(i["h"]), dev(i["x1"]), (dev(i["x2"]) if C2 else None)
    out, gn = nan_out(B, Co, T), nan_out(B, Co // 16, (T + 31) // 32, 2)
    cfg = ct.create_string_buffer(160)
    ln = i32(lengths)
    native.check(native.lib().lds_test_dconv_pair(D(dh), D(d1), D(d2), P(i["w3"]), P(i["b3"]), P(i["w1"]), P(i["b1"]), B, Cm, C1, C2, Co, T, P(ln), lvl,
                                                  tile_batch, FMT[fmt], D(out), D(gn), cfg, len(cfg), stream()))
    torch.cuda.synchronize()
    _pair_run[name, fmt] = dict(out=out.cpu().numpy(), gn=gn.cpu().numpy(), cfg=cfg.value.decode())
    return _pair_run[name, fmt]


def pair_tile(cfg):
    m = re.match(r"BM(\d+) BN(\d+) KT3\+1 S1 U0 BK(\d+)\+(\d+) NST(\d+)", cfg)
    assert m, cfg
    ks = re.search(r" KS(\d+) ", cfg)
    return tuple(int(g) for g in m.groups()) + (int(ks.group(1)) if ks else 1,)


@pytest.mark.parametrize("name,fmt", PAIR_IDS, ids=[pair_id(n, f) for n, f in PAIR_IDS])
def test_pair(name, fmt, record_margin):
    """out = conv2_k3(h) + shortcut_1x1([x1 ; x2]) + bias from one launch (reference resnet.py:636-641), every tile variant, x2 present and absent,
    T on / off the 64-column tile and T % 4 != 0, ragged batches at level 0 and 1, the latency mode's cluster split-K"""
    i, r = pair_inputs(name), pair_result(name, fmt)
    print(f"pair {name} {fmt}: {r['cfg']}")
    bm, bn, bk3, bk1, nst, ks = pair_tile(r["cfg"])
    if fmt == "f32":
        assert (bm, bk1) == PAIR[name][9] and (bn, bk3, nst) == (64, 32, 2), r["cfg"]      # a shape that lands on another tile fails here
    e = err_over_scale(r["out"], i["ref"])
    print(f"  max|got - ref| / max|ref| = {e:.3e}")
    assert_zero_tail(r["out"], i["n"])
    record_margin(e, EPS)


@pytest.mark.parametrize("name,fmt", PAIR_IDS, ids=[pair_id(n, f) for n, f in PAIR_IDS])
def test_pair_gn_mean(name, fmt, record_margin):
    """the epilogue's GroupNorm partials from the pair's k 3 + 1x1 tiles: the mean of every (16 channels x 32 frames) block over its valid frames"""
    i, r = pair_inputs(name), pair_result(name, fmt)
    e_mean, _ = gn_partial_errors(r["gn"], i["ref"], i["n"])
    print(f"pair {name} {fmt}: block mean error / max|ref| = {e_mean:.3e}")
    record_margin(e_mean, EPS)


@pytest.mark.parametrize("name,fmt", PAIR_IDS, ids=[pair_id(n, f) for n, f in PAIR_IDS])
def test_pair_gn_m2(name, fmt, record_margin):
    """... and its M2, as EPS x (error / (2 EPS A sum|y - mean| + n (EPS A)^2)): below EPS = inside the propagated output bound"""
    i, r = pair_inputs(name), pair_result(name, fmt)
    _, e_m2 = gn_partial_errors(r["gn"], i["ref"], i["n"])
    print(f"pair {name} {fmt}: EPS x worst block M2 error / bound = {e_m2:.3e}")
    record_margin(e_m2, EPS)


@pytest.mark.parametrize("fmt", list(FMT))
def test_pair_full_lengths_equal_dense(fmt):
    a, b = pair_result("full_lvl0", fmt), pair_result("dense_twin", fmt)
    assert a["cfg"] == b["cfg"]
    assert same_bits(a["out"], b["out"]) and same_bits(a["gn"], b["gn"])


@pytest.mark.parametrize("fmt", list(FMT))
def test_pair_variants_covered(fmt):
    """the configurations the cases ran with cover every fused variant of the format's launcher and a cluster split"""
    tiles = {n: pair_tile(pair_result(n, fmt)["cfg"]) for n in PAIR}
    got = {(t[0], t[1], t[2], t[3], t[4]) for t in tiles.values()}
    if fmt == "f32":      # conv_dma.hip launch_conv_dma_pair
        want = {(32, 64, 32, 64, 2), (32, 64, 32, 32, 2), (64, 64, 32, 64, 2), (64, 64, 32, 32, 2)}
    else:                 # conv_bf3.hip pair_dispatch
        want = {(32, 64, 32, 32, 2), (64, 128, 16, 32, 2), (64, 64, 16, 32, 3)}
    assert got == want, tiles
    # (b2_ks2: the shortcut's 128 channels are 2 K-steps of 64 in conv_dma and 4 of 32 in conv_bf3, which then splits four ways)
    assert (tiles["b1_ks4"][5], tiles["b2_ks2"][5], tiles["b2_ks1"][5]) == ((4, 2, 1) if fmt == "f32" else (4, 4, 1)), tiles
    assert all(t[5] == 1 for n, t in tiles.items() if not PAIR[n][8]), tiles      # no cluster outside the latency mode


def test_pair_refuses_shapes_without_a_fused_variant():
    """the entry never runs the two-launch fallback: 48 channels into the k 3 half are no multiple of its 32-channel K-step"""
    from lds import native
    B, Cm, Co, C1, T = 1, 48, 64, 64, 64
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
    h, x1, out, gn = z(B, Cm, T), z(B, C1, T), nan_out(B, Co, T), nan_out(B, Co // 16, T // 32, 2)
    w3, w1, b = np.zeros((Co, Cm, 3), np.float32), np.zeros((Co, C1, 1), np.float32), np.zeros((Co,), np.float32)
    with pytest.raises(RuntimeError, match="no fused variant"):
        native.check(native.lib().lds_test_dconv_pair(D(h), D(x1), None, P(w3), P(b), P(w1), P(b), B, Cm, C1, 0, Co, T, None, 0, 0, -1, D(out), D(gn),
                                                      None, 0, stream()))


# ==================================================================================================================================
# EPI_GELU, the encoders' geometries, lengths and GroupNorm partials inside a convolution
# ==================================================================================================================================
# name: (B, C, T, Co, K, stride, pad, options).  Options: gelu, res, ln (LayerNorm fold), gn (GroupNorm partials out), lengths (level 0) with
# lvl_in / lvl_out, n_in (explicit input lengths: HuBERT's form hands the launch its OUTPUT lengths at level 0), tile = "KT<k> S<s> ... BK<bk>"
EX = {
    "gelu_k3_c80": (2, 80, 100, 64, 3, 1, 1, dict(gelu=1, tile=(3, 1, 16))),                                  # Whisper conv1 from 80 mels: BK 16
    "gelu_k3_c128": (2, 128, 70, 128, 3, 1, 1, dict(gelu=1, tile=(3, 1, 32))),                                # ... from 128 mels
    "gelu_k3_c128_ragged": (2, 128, 70, 128, 3, 1, 1, dict(gelu=1, lengths=[70, 33], tile=(3, 1, 32))),
    "gelu_k3_s2_lvl01": (2, 128, 101, 64, 3, 2, 1, dict(gelu=1, tile=(3, 2, 32))),                            # Whisper conv2
    "gelu_k3_s2_lvl01_ragged": (3, 128, 101, 64, 3, 2, 1, dict(gelu=1, lengths=[101, 100, 34], lvl_out=1, tile=(3, 2, 32))),   # 51, 50, 17 frames out
    "gelu_k3_s2_lvl01_full": (3, 128, 101, 64, 3, 2, 1, dict(gelu=1, lengths=[101, 101, 101], lvl_out=1, tile=(3, 2, 32))),
    "gelu_k3_s2_lvl01_dense3": (3, 128, 101, 64, 3, 2, 1, dict(gelu=1, tile=(3, 2, 32))),
    "gelu_k3_s2_p0_even": (2, 64, 64, 64, 3, 2, 0, dict(gelu=1, tile=(3, 2, 32))),                            # HuBERT conv1 .. conv4
    "gelu_k3_s2_p0_odd": (2, 80, 65, 64, 3, 2, 0, dict(gelu=1, tile=(3, 2, 16))),
    "gelu_k3_s2_p0_ragged": (2, 64, 65, 64, 3, 2, 0, dict(gelu=1, n_in=[65, 38], lengths=[32, 18], tile=(3, 2, 32))),
    "gelu_k2_s2_even": (2, 64, 64, 64, 2, 2, 0, dict(gelu=1, tile=(2, 2, 32))),                               # HuBERT conv5, conv6
    "gelu_k2_s2_odd": (2, 80, 65, 64, 2, 2, 0, dict(gelu=1, tile=(2, 2, 16))),
    "gelu_k2_s2_ragged": (2, 64, 65, 64, 2, 2, 0, dict(gelu=1, n_in=[65, 37], lengths=[32, 18], tile=(2, 2, 32))),
    "gelu_1x1_ln": (2, 128, 70, 192, 1, 1, 0, dict(gelu=1, ln=1, tile=(1, 1, 32))),                           # fc1 of both encoders
    "gelu_1x1_ln_ragged": (2, 128, 70, 192, 1, 1, 0, dict(gelu=1, ln=1, lengths=[139, 66], lvl_in=1, lvl_out=1, tile=(1, 1, 32))),   # 70, 33 frames
    "gelu_k3_res": (2, 64, 50, 128, 3, 1, 1, dict(gelu=1, res=1, tile=(3, 1, 32))),
    "gelu_1x1_res_ragged": (2, 64, 50, 64, 1, 1, 0, dict(gelu=1, res=1, lengths=[50, 17], tile=(1, 1, 32))),
    "k3_gn": (2, 64, 130, 128, 3, 1, 1, dict(gn=1)),                                                          # the resnet's conv1: 32 x 64 split tile
    "k3_gn_ragged": (3, 64, 130, 128, 3, 1, 1, dict(gn=1, lengths=[130, 65, 1])),
    "k3_gn_full": (3, 64, 130, 128, 3, 1, 1, dict(gn=1, lengths=[130, 130, 130])),
    "k3_gn_dense3": (3, 64, 130, 128, 3, 1, 1, dict(gn=1)),
    "k3_gn_wide": (2, 64, 130, 704, 3, 1, 1, dict(gn=1)),                                                     # ... at a full grid: 64-row tiles
    "k3_gn_wide_ragged": (2, 64, 130, 704, 3, 1, 1, dict(gn=1, lengths=[97, 130])),
}
EX_IDS = [(n, f) for n in EX for f in FMT]
_ex_ref, _ex_run = {}, {}


def ex_inputs(name):
    if name in _ex_ref:
        return _ex_ref[name]
    B, C, T, Co, K, stride, pad, o = EX[name]
    To = (T + 2 * pad - K) // stride + 1
    key = f"ex.{C}.{T}.{Co}.{K}.{stride}.{pad}"
    x = U(key + ".x", (B, C, T), -2, 2)
    w = U(key + ".w", (Co, C, K)) / np.float32(np.sqrt(C * K))
    bias = U(key + ".b", (Co,), 0.5, 1.5)
    res = U(key + ".res", (B, Co, To), -1, 1) if o.get("res") else None
    g, be = (U(key + ".g", (C,), 0.5, 1.5), U(key + ".be", (C,), -0.5, 0.5)) if o.get("ln") else (None, None)
    if o.get("ln"):
        x = x + np.float32(0.7)      # a mean well away from zero: the fold subtracts mean * sum(W gamma)
    lengths = o.get("lengths")
    n_in = o.get("n_in") or ([valid_len(v, o.get("lvl_in", 0), T) for v in lengths] if lengths else [T] * B)
    n_out = [valid_len(v, o.get("lvl_out", 0), To) for v in lengths] if lengths else [To] * B
    x = cut(x, n_in)

    def one(xx, b):
        if o.get("ln"):
            xx = layer_norm64(xx, g, be, 1e-5)
        return epilogue64(conv64(xx, w, bias, stride, pad), o.get("gelu"), None if res is None else res[b:b + 1, :, :n_out[b]])
    ref = alone(one, n_in, n_out, To, x)
    _ex_ref[name] = dict(x=x, w=host(w), bias=host(bias), res=res, g=g, be=be, n_out=n_out, To=To, ref=ref)
    return _ex_ref[name]


def ex_call(name, fmt):
    """-> (rc, dict): the entry's return code and, when it ran, its outputs"""
    from lds import native
    B, C, T, Co, K, stride, pad, o = EX[name]
    i = ex_inputs(name)
    a = native.DConvExTest()
    dx, dres = dev(i["x"]), (dev(i["res"]) if i["res"] is not None else None)
    ln = i32(o.get("lengths"))
    a.x1, a.x2, a.C1, a.C2, a.T = dx.data_ptr(), None, C, 0, T
    a.w, a.bias, a.Co, a.K, a.stride, a.pad = i["w"].ctypes.data, i["bias"].ctypes.data, Co, K, stride, pad
    a.res = dres.data_ptr() if dres is not None else None
    a.epilogue = 3 if o.get("gelu") else 0
    a.lengths = ln.ctypes.data if ln is not None else None
    a.lvl_in, a.lvl_out = o.get("lvl_in", 0), o.get("lvl_out", 0)
    a.ln_gamma = i["g"].ctypes.data if i["g"] is not None else None
    a.ln_beta = i["be"].ctypes.data if i["be"] is not None else None
    a.ln_eps, a.tile_batch, a.fmt = 1e-5, 0, FMT[fmt]
    To = i["To"]
    out = nan_out(B, Co, To)
    gn = nan_out(B, Co // 16, (To + 31) // 32, 2) if o.get("gn") else None
    cfg = ct.create_string_buffer(160)
    rc = native.lib().lds_test_dconv_ex(ct.byref(a), D(out), D(gn), B, cfg, len(cfg), stream())
    torch.cuda.synchronize()
    if rc != 0:
        return rc, dict(error=native.lib().lds_last_error().decode())
    return rc, dict(out=out.cpu().numpy(), gn=gn.cpu().numpy() if gn is not None else None, cfg=cfg.value.decode())


def ex_result(name, fmt):
    if (name, fmt) not in _ex_run:
        _ex_run[name, fmt] = ex_call(name, fmt)
    return _ex_run[name, fmt]


def split_has_mode(name):
    """launch_conv_bf3 has no plain-GELU epilogue (and with it none of the k 2 / pad 0 geometries): it must refuse, not compute something else"""
    return not EX[name][7].get("gelu")


@pytest.mark.parametrize("name,fmt", EX_IDS, ids=[f"{n}-{f}" for n, f in EX_IDS])
def test_dconv_ex(name, fmt, record_margin):
    """GELU on k 3 / k 3 stride 2 (pad 1 and 0) / k 2 stride 2 / the LayerNorm fold / before a residual; lengths at lvl_in -> lvl_out; k 3 with
    GroupNorm partials.  The split-plane launcher runs the modes it has and refuses the others."""
    o = EX[name][7]
    i = ex_inputs(name)
    rc, r = ex_result(name, fmt)
    if fmt != "f32" and not split_has_mode(name):
        assert rc != 0 and "conv_bf3 launch failed" in r["error"], (rc, r)      # the gap, on record
        return
    assert rc == 0, r
    print(f"ex {name} {fmt}: {r['cfg']}")
    if fmt == "f32" and "tile" in o:
        m = re.match(r"BM\d+ BN\d+ KT(\d+) S(\d+) U0 BK(\d+) NST\d+ GELU ", r["cfg"])
        assert m and tuple(int(g) for g in m.groups()) == o["tile"], r["cfg"]
    e = err_over_scale(r["out"], i["ref"])
    print(f"  max|got - ref| / max|ref| = {e:.3e}")
    assert_zero_tail(r["out"], i["n_out"])
    record_margin(e, EPS)


EX_GN_IDS = [(n, f) for n, f in EX_IDS if EX[n][7].get("gn")]


@pytest.mark.parametrize("name,fmt", EX_GN_IDS, ids=[f"{n}-{f}" for n, f in EX_GN_IDS])
def test_dconv_ex_gn_mean(name, fmt, record_margin):
    """GroupNorm partials from k 3 tiles (the resnet's conv1), over the valid frames only: block means"""
    i, (rc, r) = ex_inputs(name), ex_result(name, fmt)
    assert rc == 0, r
    e_mean, _ = gn_partial_errors(r["gn"], i["ref"], i["n_out"])
    print(f"ex {name} {fmt}: block mean error / max|ref| = {e_mean:.3e}")
    record_margin(e_mean, EPS)


@pytest.mark.parametrize("name,fmt", EX_GN_IDS, ids=[f"{n}-{f}" for n, f in EX_GN_IDS])
def test_dconv_ex_gn_m2(name, fmt, record_margin):
    i, (rc, r) = ex_inputs(name), ex_result(name, fmt)
    assert rc == 0, r
    _, e_m2 = gn_partial_errors(r["gn"], i["ref"], i["n_out"])
    print(f"ex {name} {fmt}: EPS x worst block M2 error / bound = {e_m2:.3e}")
    record_margin(e_m2, EPS)


@pytest.mark.parametrize("full,dense,fmt", [("gelu_k3_s2_lvl01_full", "gelu_k3_s2_lvl01_dense3", "f32")] + [("k3_gn_full", "k3_gn_dense3", f) for f in FMT])
def test_dconv_ex_full_lengths_equal_dense(full, dense, fmt):
    (rca, a), (rcb, b) = ex_result(full, fmt), ex_result(dense, fmt)
    assert rca == 0 and rcb == 0 and a["cfg"] == b["cfg"]
    assert same_bits(a["out"], b["out"])
    assert a["gn"] is None or same_bits(a["gn"], b["gn"])


def test_dconv_ex_variants_covered():
    """every GELU instantiation family of launch_conv_dma ran: k 1 / k 3 stride 1, k 3 / k 2 stride 2, each with 32- and (where a case has 80
    channels) 16-channel K-steps; the GroupNorm cases ran on the split-K 32-row tile and on 64-row tiles"""
    got = set()
    for n in EX:
        rc, r = ex_result(n, "f32")
        assert rc == 0, (n, r)
        m = re.match(r"BM(\d+) BN\d+ KT(\d+) S(\d+) U0 BK(\d+) NST\d+( GELU)? ", r["cfg"])
        assert m, r["cfg"]
        got.add((int(m.group(2)), int(m.group(3)), int(m.group(4))) if m.group(5) else ("gn", int(m.group(1))))
    assert got >= {(3, 1, 16), (3, 1, 32), (3, 2, 32), (3, 2, 16), (2, 2, 32), (2, 2, 16), (1, 1, 32), ("gn", 32), ("gn", 64)}, got


# ==================================================================================================================================
# the vocoder's upsamplers on conv_dma
# ==================================================================================================================================
UPS_SHAPES = [(128, 64, 4, 2), (128, 64, 16, 8), (256, 128, 32, 16)]
UPS_T = [1, 31, 127, 128, 129]      # T + 1 columns: on, at and past the 128-column tile
UPS_IDS = [(s, T) for s in UPS_SHAPES for T in UPS_T]
_ups_ref, _ups_run = {}, {}


def ups_inputs(shape, T):
    if (shape, T) in _ups_ref:
        return _ups_ref[shape, T]
    Ci, Co, K, s = shape
    B, pad = 2, (K - s + 1) // 2
    Tn = (T - 1) * s - 2 * pad + K
    key = f"ups.{Ci}.{Co}.{K}.{T}"
    x = U(key + ".x", (B, Ci, T), -2, 2)
    w = U(key + ".w", (Ci, Co, K)) / np.float32(np.sqrt(Ci * K / s))
    bias = U(key + ".b", (Co,), 0.5, 1.5)
    n_in = [T, max(1, T // 2)]
    n_out = [(n - 1) * s - 2 * pad + K for n in n_in]      # what the generator's driver derives

    def one(xx, b):
        return conv_transpose64(lrelu64(xx.astype(np.float64)), w, bias, s, pad)
    ref = alone(one, n_in, n_out, Tn, x)
    act = lrelu64(ref)
    _ups_ref[shape, T] = dict(x=x, w=host(w), bias=host(bias), n_in=n_in, n_out=n_out, Tn=Tn, ref=ref, act=act)
    return _ups_ref[shape, T]


def ups_call(shape, T, x, n_in, n_out):
    from lds import native
    Ci, Co, K, s = shape
    i = ups_inputs(shape, T)
    dx = dev(x)
    out, act = nan_out(2, Co, i["Tn"]), nan_out(2, Co, i["Tn"])
    cfg = ct.create_string_buffer(160)
    li, lo = i32(n_in), i32(n_out)
    native.check(native.lib().lds_test_voc_ups(D(dx), P(i["w"]), P(i["bias"]), 2, Ci, Co, T, K, s, P(li), P(lo), D(out), D(act), cfg, len(cfg), stream()))
    torch.cuda.synchronize()
    return dict(out=out.cpu().numpy(), act=act.cpu().numpy(), cfg=cfg.value.decode())


def ups_result(shape, T):
    if (shape, T) not in _ups_run:
        i = ups_inputs(shape, T)
        _ups_run[shape, T] = ups_call(shape, T, cut(i["x"], i["n_in"]), i["n_in"], i["n_out"])
    return _ups_run[shape, T]


@pytest.mark.parametrize("shape,T", UPS_IDS, ids=[f"{s[0]}-{s[1]}-k{s[2]}-s{s[3]}-T{T}" for s, T in UPS_IDS])
def test_voc_ups(shape, T, record_margin):
    """x -> LeakyReLU K4P copy -> polyphase ConvTranspose1d on conv_dma (launch_to_k4p_act + launch_k4p_zero_pads + ph_log2 / ph_tpad / ph_Tout,
    store_phases), a ragged batch of two; the raw output"""
    i, r = ups_inputs(shape, T), ups_result(shape, T)
    print(f"ups {shape} T {T}: {r['cfg']}")
    assert re.match(r"BM64 BN128 KT2 S1 U0 BK16 NST2 D1 ", r["cfg"]), r["cfg"]
    e = err_over_scale(r["out"], i["ref"])
    print(f"  raw: max|got - ref| / max|ref| = {e:.3e}")
    assert_zero_tail(r["out"], i["n_out"])
    record_margin(e, EPS)


@pytest.mark.parametrize("shape,T", UPS_IDS, ids=[f"{s[0]}-{s[1]}-k{s[2]}-s{s[3]}-T{T}" for s, T in UPS_IDS])
def test_voc_ups_activated(shape, T, record_margin):
    """... and its LeakyReLU'd twin from the same store"""
    i, r = ups_inputs(shape, T), ups_result(shape, T)
    e = err_over_scale(r["act"], i["act"])
    print(f"ups {shape} T {T}: activated: max|got - ref| / max|ref| = {e:.3e}")
    assert_zero_tail(r["act"], i["n_out"])
    record_margin(e, EPS)


@pytest.mark.parametrize("shape,T", [(UPS_SHAPES[0], 129), (UPS_SHAPES[1], 31), (UPS_SHAPES[2], 128)])
@pytest.mark.parametrize("poison", [float("nan"), float("inf"), float("-inf"), 1e30, -1e30])
def test_voc_ups_does_not_read_beyond_lengths_in(shape, T, poison):
    """input at and beyond lengths_in is not read: any value there gives the bits of the zero-padded run"""
    i, r = ups_inputs(shape, T), ups_result(shape, T)
    x = i["x"].copy()
    for b, n in enumerate(i["n_in"]):
        x[b, :, n:] = poison
    p = ups_call(shape, T, x, i["n_in"], i["n_out"])
    assert same_bits(p["out"], r["out"]) and same_bits(p["act"], r["act"])


@pytest.mark.parametrize("shape,T", [(UPS_SHAPES[0], 127), (UPS_SHAPES[1], 129), (UPS_SHAPES[2], 31)])
def test_voc_ups_full_lengths_equal_dense(shape, T):
    i = ups_inputs(shape, T)
    dense = ups_call(shape, T, i["x"], None, None)
    full = ups_call(shape, T, i["x"], [T, T], [i["Tn"], i["Tn"]])
    assert same_bits(dense["out"], full["out"]) and same_bits(dense["act"], full["act"])
    ref = conv_transpose64(lrelu64(i["x"].astype(np.float64)), i["w"], i["bias"], shape[3], (shape[2] - shape[3] + 1) // 2)
    assert err_over_scale(dense["out"], ref) < EPS
