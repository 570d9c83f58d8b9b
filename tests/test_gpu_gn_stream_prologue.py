"""gn_stream_kernel with everything requested at its top (csrc/k4p_ops.hip): every instantiation and every path of its statistics --
<1> (T <= 128), <2> (T <= 256), <4> with a second chunk and more than 64 partials (T = 600 at 64 channels per group), and the cold
rounds beyond 128 partials (T = 1056) -- with 16 / 32 / 64 channels per group, one and two sources, scale/shift and SiLU on and off,
against a float64 GroupNorm with the tolerance of tests/test_gpu_k4p.py test_gn_apply."""
import ctypes as ct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def relmax(a, b):
    return float(np.abs(a - b).max() / max(1e-30, np.abs(b).max()))


def U(name, shape, lo=-1.0, hi=1.0):
    from lds import init_weights
    return init_weights.uniform("gnpro." + name, shape, 13, lo, hi)


def stream():
    return ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def group_norm64(x, g, be, groups, eps):
    B, C, T = x.shape
    xg = x.astype(np.float64).reshape(B, groups, -1)
    mu, var = xg.mean(-1, keepdims=True), xg.var(-1, keepdims=True)
    return ((xg - mu) / np.sqrt(var + eps)).reshape(B, C, T) * g.astype(np.float64)[None, :, None] + be.astype(np.float64)[None, :, None]


CASES = [(C1, C2, groups, T, 2) for (C1, C2, groups) in [(64, 0, 4), (32, 32, 2), (512, 0, 8)] for T in (1, 31, 33, 128, 130, 256, 600)]
CASES.append((512, 0, 8, 1056, 1))      # 4 x 33 = 132 partials per group


@pytest.mark.parametrize("C1,C2,groups,T,B", CASES)
@pytest.mark.parametrize("silu", [0, 1])
@pytest.mark.parametrize("ss", [False, True])
def test_gn_stream(C1, C2, groups, T, B, silu, ss):
    from lds import native
    C = C1 + C2
    x1 = U(f"{C1}.{C2}.{T}.x1", (B, C1, T), -2, 2) + np.float32(0.7)
    x2 = U(f"{C1}.{C2}.{T}.x2", (B, C2, T), -3, 1) if C2 else None
    g, be = U(f"{C}.g", (C,), 0.5, 1.5), U(f"{C}.b", (C,), -0.5, 0.5)
    sst = U(f"{C}.ss", (B, 2 * C), -0.5, 0.5) if ss else None
    out = torch.full((B, C, T), float("nan"), dtype=torch.float32, device="cuda")
    d1, d2, dss = dev(x1), (dev(x2) if C2 else None), (dev(sst) if ss else None)
    native.check(native.lib().lds_test_gn_apply(ct.c_void_p(d1.data_ptr()), ct.c_void_p(d2.data_ptr()) if C2 else None, C1, C2, T, groups,
                                                ct.c_float(1e-5), ct.c_void_p(g.ctypes.data), ct.c_void_p(be.ctypes.data),
                                                ct.c_void_p(dss.data_ptr()) if ss else None, silu, ct.c_void_p(out.data_ptr()), B, stream()))
    torch.cuda.synchronize()
    x = x1 if x2 is None else np.concatenate([x1, x2], axis=1)
    ref = group_norm64(x, g, be, groups, 1e-5)
    if ss:
        ref = ref * (1 + sst[:, :C, None].astype(np.float64)) + sst[:, C:, None].astype(np.float64)
    if silu:
        ref = ref / (1 + np.exp(-ref))
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    assert relmax(got, ref) < 1e-5, relmax(got, ref)
