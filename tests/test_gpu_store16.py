"""The K4P outputs of conv_dma and of the attention leave as 16-byte entries put together from two lane halves (csrc/k4p.h
k4p_tile_entries), and single-tile waves request their epilogue operands behind the first tiles' DMAs with counted waits (csrc/conv_dma.hip
late_loads / wait_younger).  A misplaced entry, a swap under a partial lane mask or a wait that counts one operation too many gives an O(1)
error or leaves a NaN, so every case here fills the output with NaN, checks EVERY element of what the entry point returns against a float64
numpy computation at the tolerance tests/test_gpu_k4p.py holds the same entry point to (2e-5 of max|ref| for the convolutions, 3e-5 for the
attention), and checks that frames at and beyond a ragged length and the VT tail are exactly zero.  The K4P buffer the kernel wrote is
read as well, through lds_test_tap_k4p (include/lds_test.h), which fills it with NaN before the launch and returns it as the kernel left
it: both pad frames of every row must be exactly 0, nothing may be NaN, and its frames must be the values the entry point returned.

Shapes: B = 2 and the smallest at which the paths differ -- T = 37 (one ragged 64-frame block, T % 4 = 1), 64, 70 and 130 (several frame
blocks; with the deep reductions several K-steps through the 2-deep ring, so that the wait at the first tile boundary is the adjusted one)."""
import ctypes as ct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EPS = 2e-5


def U(name, shape, lo=-1.0, hi=1.0):
    from lds import init_weights
    return init_weights.uniform("s16." + name, shape, 13, lo, hi)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def D(t):
    return ct.c_void_p(t.data_ptr()) if t is not None else None


def P(a):
    return ct.c_void_p(a.ctypes.data) if a is not None else None


def stream():
    return ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def nan_out(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def conv64(x, w, bias=None, pad=0):
    """float64 convolution, stride 1: x [B][Ci][T], w [Co][Ci][K]"""
    B, Ci, T = x.shape
    Co, _, K = w.shape
    xp = np.zeros((B, Ci, T + 2 * pad), np.float64)
    xp[:, :, pad:pad + T] = x
    To = T + 2 * pad - K + 1
    y = np.zeros((B, Co, To), np.float64)
    for k in range(K):
        y += np.einsum("oc,bct->bot", w[:, :, k].astype(np.float64), xp[:, :, k:k + To])
    if bias is not None:
        y += bias.astype(np.float64)[None, :, None]
    return y


class Tap:
    """with Tap(B, C, T) as t: <one call of a K4P test entry>; t.check(got) afterwards"""

    def __init__(self, B, C, T):
        self.B, self.C, self.T = B, C, T
        self.buf = nan_out(B * C * (T + 2))

    def __enter__(self):
        from lds import native
        native.check(native.lib().lds_test_tap_k4p(D(self.buf), self.buf.numel()))
        return self

    def __exit__(self, *exc):
        from lds import native
        native.check(native.lib().lds_test_tap_k4p(None, 0))
        return False

    def check(self, got):
        """the raw tensor [B][C/8][2][T + 2][4]: pad frames exactly 0, no NaN, frames 0 .. T-1 bit for bit what the entry point returned"""
        B, C, T = self.B, self.C, self.T
        torch.cuda.synchronize()
        raw = self.buf.cpu().numpy().reshape(B, C // 8, 2, T + 2, 4)
        assert np.isfinite(raw).all(), "an element of the K4P buffer was left NaN"
        assert (raw[:, :, :, 0, :] == 0).all(), "left pad frame not zero"
        assert (raw[:, :, :, T + 1, :] == 0).all(), "right pad frame not zero"
        # channel 8 q + 2 j + h at [q][h][t + 1][j]
        plain = raw[:, :, :, 1:T + 1, :].transpose(0, 1, 4, 2, 3).reshape(B, C, T)
        assert np.array_equal(plain, got[:, :C]), "the K4P buffer and the returned tensor differ"


def check_all(got, ref, lengths=None, eps=EPS):
    assert got.shape == ref.shape
    assert np.isfinite(got).all(), "an element was left NaN"
    if lengths is not None:
        for b, n in enumerate(lengths):
            assert (got[b, :, n:] == 0).all(), f"utterance {b}: nonzero frame at or beyond its length {n}"
    e = float(np.abs(got - ref).max() / np.abs(ref).max())
    print(f"  max|got - ref| / max|ref| = {e:.3e}")
    assert e < eps, e


def run_ex(x, w, bias=None, K=1, pad=0, res=None, lengths=None, ln=None, tile_batch=0, want_gn=False):
    from lds import native
    B, C, T = x.shape
    Co = w.shape[0]
    a = native.DConvExTest()
    dx, dres = dev(x), (dev(res) if res is not None else None)
    wk = np.ascontiguousarray(w, dtype=np.float32)
    ln_i = np.asarray(lengths, dtype=np.int32) if lengths is not None else None
    a.x1, a.x2, a.C1, a.C2, a.T = dx.data_ptr(), None, C, 0, T
    a.w, a.bias, a.Co, a.K, a.stride, a.pad = wk.ctypes.data, (bias.ctypes.data if bias is not None else None), Co, K, 1, pad
    a.res, a.epilogue = (dres.data_ptr() if dres is not None else None), 0
    a.lengths, a.lvl_in, a.lvl_out = (ln_i.ctypes.data if ln_i is not None else None), 0, 0
    if ln is not None:
        a.ln_gamma, a.ln_beta, a.ln_eps = ln[0].ctypes.data, ln[1].ctypes.data, 1e-5
    a.tile_batch, a.fmt = tile_batch, -1
    out = nan_out(B, Co, T)
    gn = nan_out(B, Co // 16, (T + 31) // 32, 2) if want_gn else None
    cfg = ct.create_string_buffer(160)
    with Tap(B, Co, T) as tap:
        native.check(native.lib().lds_test_dconv_ex(ct.byref(a), D(out), D(gn), B, cfg, len(cfg), stream()))
    torch.cuda.synchronize()
    print(f"  {cfg.value.decode()}")
    got = out.cpu().numpy()
    tap.check(got)
    return got, (gn.cpu().numpy() if want_gn else None), cfg.value.decode()


def masked(x, lengths):
    x = x.copy()
    for b, n in enumerate(lengths):
        x[b, :, n:] = 0
    return x


@pytest.mark.parametrize("T", [37, 64])
def test_split_tile_residual(T):
    """1x1, 64 -> 64 channels at B = 2: the 32 x 64 split-K tile, whose two joining waves store; residual and bias come from late_loads()"""
    x, w, b = U(f"sp{T}.x", (2, 64, T), -2, 2), U(f"sp{T}.w", (64, 64, 1)) / np.float32(8), U(f"sp{T}.b", (64,))
    res = U(f"sp{T}.r", (2, 64, T))
    got, _, cfg = run_ex(x, w, b, res=res)
    assert cfg.startswith("BM32 BN64"), cfg
    check_all(got, conv64(x, w, b) + res)


def test_split_tile_layernorm_partials():
    """the same tile writing per-frame LayerNorm partials, consumed by a LayerNorm-folded convolution (lds_test_ln_chain_k4p)"""
    from lds import native
    B, C, Co, T = 2, 64, 64, 37
    x = U("lnp.x", (B, C, T), -2, 2)
    w1 = (U("lnp.w1", (C, C)) / np.float32(8)).astype(np.float32)
    w2 = (U("lnp.w2", (Co, C)) / np.float32(8)).astype(np.float32)
    g, be = U("lnp.g", (C,), 0.5, 1.5), U("lnp.b", (C,), -0.5, 0.5)
    mid, out = nan_out(B, C, T), nan_out(B, Co, T)
    dx = dev(x)
    with Tap(B, Co, T) as tap:
        native.check(native.lib().lds_test_ln_chain_k4p(D(dx), P(w1), P(w2), P(g), P(be), ct.c_float(1e-5), D(mid), D(out), B, C, Co, T, stream()))
    torch.cuda.synchronize()
    tap.check(out.cpu().numpy())
    rmid = conv64(x, w1[:, :, None])
    mu, var = rmid.mean(1, keepdims=True), rmid.var(1, keepdims=True)
    rn = (rmid - mu) / np.sqrt(var + 1e-5) * g[None, :, None] + be[None, :, None]
    check_all(mid.cpu().numpy(), rmid)
    check_all(out.cpu().numpy(), conv64(rn, w2[:, :, None]))


def test_edge_tile_k3_groupnorm_partials():
    """k 3, 64 -> 96 channels (Co no multiple of 64: the last M-block is half empty), T = 70, with the epilogue's GroupNorm partials"""
    B, T, Co = 2, 70, 96
    x, w, b = U("k3.x", (B, 64, T), -2, 2), U("k3.w", (Co, 64, 3)) / np.float32(np.sqrt(192)), U("k3.b", (Co,), 0.5, 1.5)
    got, gn, _ = run_ex(x, w, b, K=3, pad=1, want_gn=True)
    ref = conv64(x, w, b, pad=1)
    check_all(got, ref)
    assert np.isfinite(gn).all()
    A = np.abs(ref).max()
    for blk in range((T + 31) // 32):
        t = ref[:, :, blk * 32:min(T, blk * 32 + 32)].reshape(B, Co // 16, 16, -1)
        mean = t.mean((2, 3))
        m2 = ((t - mean[:, :, None, None]) ** 2).sum((2, 3))
        assert np.abs(gn[:, :, blk, 0] - mean).max() < EPS * A
        bound = 2 * EPS * A * np.abs(t - mean[:, :, None, None]).sum((2, 3)) + t[0, 0].size * (EPS * A) ** 2
        assert (np.abs(gn[:, :, blk, 1] - m2) <= bound + 1e-6).all()


def test_pair_kernel():
    """the fused resnet tail 64 + 64 -> 64 at T = 37: two reductions, then ONE epilogue whose operands the second phase requests"""
    from lds import native
    B, Cm, C1, C2, Co, T = 2, 64, 64, 64, 64, 37
    h, x1, x2 = U("pr.h", (B, Cm, T), -2, 2), U("pr.x1", (B, C1, T), -2, 2), U("pr.x2", (B, C2, T), -2, 2)
    w3, w1 = U("pr.w3", (Co, Cm, 3)) / np.float32(np.sqrt(3 * Cm)), U("pr.w1", (Co, C1 + C2, 1)) / np.float32(np.sqrt(C1 + C2))
    b3, b1 = U("pr.b3", (Co,)), U("pr.b1", (Co,))
    out, gn = nan_out(B, Co, T), nan_out(B, Co // 16, (T + 31) // 32, 2)
    dh, d1, d2 = dev(h), dev(x1), dev(x2)
    cfg = ct.create_string_buffer(160)
    with Tap(B, Co, T) as tap:
        native.check(native.lib().lds_test_dconv_pair(D(dh), D(d1), D(d2), P(w3), P(b3), P(w1), P(b1), B, Cm, C1, C2, Co, T, None, 0, 0, -1, D(out), D(gn),
                                                      cfg, len(cfg), stream()))
    torch.cuda.synchronize()
    tap.check(out.cpu().numpy())
    print(f"  {cfg.value.decode()}")
    ref = conv64(h, w3, b3, pad=1) + conv64(np.concatenate([x1, x2], axis=1), w1, b1)
    check_all(out.cpu().numpy(), ref)
    assert np.isfinite(gn.cpu().numpy()).all()


@pytest.mark.parametrize("T", [37, 130])
@pytest.mark.parametrize("C", [64, 96, 128])
def test_qkv_layernorm_fold(C, T):
    """the QKV projection's LayerNorm fold (64 x 64 / 128 x 64 tiles, column statistics fetched between the first DMAs and the first wait),
    dense and with lens = [T, T - 33]"""
    B = 2
    x = U(f"qln{C}.{T}.x", (B, C, T), -2, 2) + np.float32(0.3)
    w = U(f"qln{C}.{T}.w", (3 * C, C, 1)) / np.float32(np.sqrt(C))
    b = U(f"qln{C}.{T}.b", (3 * C,))
    g, be = U(f"qln{C}.{T}.g", (C,), 0.5, 1.5), U(f"qln{C}.{T}.be", (C,), -0.5, 0.5)

    def ref_of(xx):
        mu, var = xx.astype(np.float64).mean(1, keepdims=True), xx.astype(np.float64).var(1, keepdims=True)
        return conv64((xx - mu) / np.sqrt(var + 1e-5) * g[None, :, None] + be[None, :, None], w, b)

    got, _, _ = run_ex(x, w, b, ln=(g, be))
    check_all(got, ref_of(x))
    lengths = [T, T - 33]
    xm = masked(x, lengths)
    got, _, _ = run_ex(xm, w, b, ln=(g, be), lengths=lengths)
    check_all(got, masked(ref_of(xm), lengths), lengths=lengths)


@pytest.mark.parametrize("T", [37, 130])
@pytest.mark.parametrize("C", [64, 96, 128])
def test_qkv_value_layout(C, T):
    """q and k rows leave as 16-byte K4P entries, v rows in the attention's VT layout with frames T .. ceil4(T) - 1 exactly zero (two heads:
    D = 32, 48, 64)"""
    from lds import native
    B, heads = 2, 2
    Dh = C // heads
    x = U(f"vt{C}.{T}.x", (B, 64, T), -2, 2)
    w = U(f"vt{C}.{T}.w", (3 * C, 64, 1)) / np.float32(8)
    ref = conv64(x, w)
    T4 = (T + 3) // 4 * 4
    a = native.DConvTest()
    dx = dev(x)
    wk = np.ascontiguousarray(w, dtype=np.float32)
    a.x1, a.x2, a.C1, a.C2, a.T = dx.data_ptr(), None, 64, 0, T
    a.w, a.bias, a.Co, a.K, a.stride, a.pad, a.ups = wk.ctypes.data, None, 3 * C, 1, 1, 0, 0
    a.res, a.epilogue, a.plain_out, a.v_split, a.cfg = None, 0, 0, Dh, 0
    out = nan_out(B * 2 * C * T + B * C * T4)
    with Tap(B, 2 * C, T) as tap:
        native.check(native.lib().lds_test_dconv(ct.byref(a), D(out), None, B, stream()))
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    tap.check(o[:B * 2 * C * T].reshape(B, 2 * C, T))
    check_all(o[:B * 2 * C * T].reshape(B, 2 * C, T), ref[:, :2 * C])
    vt = o[B * 2 * C * T:].reshape(B, heads, T4 // 4, Dh, 4).transpose(0, 1, 3, 2, 4).reshape(B, C, T4)
    assert np.isfinite(vt).all()
    assert (vt[:, :, T:] == 0).all()
    check_all(vt[:, :, :T], ref[:, 2 * C:])


def test_ff1_geglu():
    """FF1: 64 -> 512 rows, value * gelu(gate) in the epilogue of a two-tile wave (128-row tiles), T = 37"""
    from lds import native
    from math import erf
    B, T = 2, 37
    x = U("ff.x", (B, 64, T), -2, 2)
    w, b = U("ff.w", (512, 64, 1)) / np.float32(8), U("ff.b", (512,))
    a = native.DConvTest()
    dx = dev(x)
    wk, bk = np.ascontiguousarray(w, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    a.x1, a.x2, a.C1, a.C2, a.T = dx.data_ptr(), None, 64, 0, T
    a.w, a.bias, a.Co, a.K, a.stride, a.pad, a.ups = wk.ctypes.data, bk.ctypes.data, 512, 1, 1, 0, 0
    a.res, a.epilogue, a.plain_out, a.v_split, a.cfg = None, 1, 0, 0, 0
    out = nan_out(B, 256, T)
    with Tap(B, 256, T) as tap:
        native.check(native.lib().lds_test_dconv(ct.byref(a), D(out), None, B, stream()))
    torch.cuda.synchronize()
    tap.check(out.cpu().numpy())
    y = conv64(x, w, b)
    val, gate = y[:, :256], y[:, 256:]
    ref = val * 0.5 * gate * (1 + np.vectorize(erf)(gate / np.sqrt(2.0)))
    check_all(out.cpu().numpy(), ref)


def test_cluster_split_k():
    """latency mode at B = 1 on a 1x1 that really splits: 256 -> 64 channels is four K-steps of the 32 x 64 tile (BK 64), which two workgroups
    share (a share keeps two K-steps), so every workgroup issues its late loads, one of them leaves in cluster_join and the one that
    arrives last adds the residual and stores the 16-byte entries.  The configuration that ran must name the cluster split (KS)."""
    T = 64
    x, w, b = U("cl.x", (1, 256, T), -2, 2), U("cl.w", (64, 256, 1)) / np.float32(16), U("cl.b", (64,))
    res = U("cl.r", (1, 64, T))
    got, _, cfg = run_ex(x, w, b, res=res, tile_batch=1)
    assert cfg.startswith("BM32 BN64") and " KS" in cfg, cfg
    check_all(got, conv64(x, w, b) + res)


@pytest.mark.parametrize("T", [37, 130])
@pytest.mark.parametrize("Dh", [32, 48, 64])
def test_attention_store(Dh, T):
    """attention output tiles of 32 / 48 / 64 channels per head (48: half of the second tile's 8-channel blocks exist)"""
    from lds import native
    B, heads = 2, 2
    C = heads * Dh
    qkv = U(f"att{Dh}.{T}", (B, 3 * C, T), -1.5, 1.5)
    out = nan_out(B, C, T)
    dq = dev(qkv)
    with Tap(B, C, T) as tap:
        native.check(native.lib().lds_test_attention_k4p(D(dq), D(out), B, C, T, heads, stream()))
    torch.cuda.synchronize()
    tap.check(out.cpu().numpy())
    q, k, v = [qkv[:, i * C:(i + 1) * C].reshape(B, heads, Dh, T).astype(np.float64) for i in range(3)]
    s = np.einsum("bhdq,bhdk->bhqk", q, k) / np.sqrt(Dh)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    ref = np.einsum("bhqk,bhdk->bhdq", p, v).reshape(B, C, T)
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    assert np.abs(got - ref).max() < 3e-5 * np.abs(ref).max() + 1e-6
