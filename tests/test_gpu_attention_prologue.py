"""attention_k4p_kernel with its query fragments loaded unconditionally in front of the first K/V tile (csrc/attention_k4p.hip): every
variant the launcher can choose at 8 heads -- one-wave (T <= 32), KS = 2 (T <= 384) and 128-query workgroups (T >= 385), the latency
mode's KS = 4, exact fp32 and split-fp16 -- at head dims 32 / 48 / 64 against a float64 softmax attention, with the tolerance
tests/test_gpu_k4p.py applies to the same entry points.  The ragged cases poison q, k and v beyond each clip's length with NaN (the entry
zeroes v there, as the QKV convolution writes it): valid queries match the reference over the clip's own keys, queries beyond the
length are exactly zero, nothing is NaN."""
import ctypes as ct
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HEADS = 8


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()      # (a copy: the cached inputs are read-only)


def stream():
    return ct.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def inputs(C, T, B):
    from lds import init_weights
    qkv = init_weights.uniform(f"attpro.{C}.{T}.{B}", (B, 3 * C, T), 11, -1.5, 1.5)
    qkv.setflags(write=False)
    return qkv


def attention64(qkv, C, n):
    """float64 softmax(q k^T / sqrt(d)) v of one clip [3C, T] over its first n frames -> [C, n]"""
    d = C // HEADS
    q, k, v = [qkv[i * C:(i + 1) * C, :n].reshape(HEADS, d, n).astype(np.float64) for i in range(3)]
    s = np.matmul(q.transpose(0, 2, 1), k) / np.sqrt(d)
    s -= s.max(-1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(-1, keepdims=True)
    return np.matmul(v, p.transpose(0, 2, 1)).reshape(C, n)


@functools.lru_cache(maxsize=None)
def reference(C, T, B):
    ref = np.stack([attention64(inputs(C, T, B)[b], C, T) for b in range(B)])
    ref.setflags(write=False)
    return ref


def close(got, ref):
    return np.abs(got - ref).max() < 3e-5 * np.abs(ref).max() + 1e-6


# one-wave: 1, 31, 32; KS = 2: 33, 65, 130, 384; 128-query workgroups: 385, 512
@pytest.mark.parametrize("T", [1, 31, 32, 33, 65, 130, 384, 385, 512])
@pytest.mark.parametrize("D", [32, 48, 64])
@pytest.mark.parametrize("math", ["f32", "f16x2", "f32-lat", "f16x2-lat"])
def test_attention_variants(D, T, math):
    from lds import native
    B, C = 2, D * HEADS
    dq = dev(inputs(C, T, B))
    out = torch.full((B, C, T), float("nan"), dtype=torch.float32, device="cuda")
    P = lambda t: ct.c_void_p(t.data_ptr())
    if math.endswith("-lat"):
        native.check(native.lib().lds_test_attention_latency(P(dq), P(out), B, C, T, HEADS, 1 if math.startswith("f16") else 0, stream()))
    else:
        fn = native.lib().lds_test_attention_k4p if math == "f32" else native.lib().lds_test_attention_f16math
        native.check(fn(P(dq), P(out), B, C, T, HEADS, stream()))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    assert close(got, reference(C, T, B))


@pytest.mark.parametrize("T,lens", [(32, (32, 1, 31, 17)), (65, (65, 34, 33, 1)), (130, (130, 99, 33, 1)), (512, (512, 481, 33, 1))])
@pytest.mark.parametrize("D", [32, 48, 64])
@pytest.mark.parametrize("math", ["f32", "f16x2", "f32-lat"])
def test_attention_ragged_nan_poisoned(D, T, lens, math):
    from lds import native
    B, C = len(lens), D * HEADS
    qkv = inputs(C, T, B).copy()
    for b, n in enumerate(lens):
        qkv[b, :, n:] = np.nan
    dq = dev(qkv)
    out = torch.full((B, C, T), float("nan"), dtype=torch.float32, device="cuda")
    hl = np.asarray(lens, dtype=np.int32)
    native.check(native.lib().lds_test_attention_ragged(ct.c_void_p(dq.data_ptr()), ct.c_void_p(hl.ctypes.data), ct.c_void_p(out.data_ptr()), B, C, T, HEADS,
                                                        1 if math.startswith("f16") else 0, 1 if math.endswith("-lat") else 0, stream()))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert not np.isnan(got).any()
    for b, n in enumerate(lens):
        assert close(got[b, :, :n], attention64(qkv[b], C, n)), (b, n)
        assert (got[b, :, n:] == 0).all(), (b, n)
