"""The ragged VAE encoder (Vocoder.extract_ragged, include/lds.h lds_vae_encoder_forward_ragged) without a GPU: the public signatures,
the Python argument validation, and the C entry's argument validation on the sanitizer build of the host side (make asan), where nothing
can be launched: every refusal must come before anything is enqueued."""
import glob
import inspect
import os
import re
import subprocess
import sys

import pytest

from conftest import PKG, ROOT


def test_extract_ragged_signatures():
    from diffusion.vocoder import Vocoder
    from encoder.hifi_vaegan.hifi_vaegan import Hifi_VAEGAN
    sig = inspect.signature(Hifi_VAEGAN.extract_ragged)
    pos = [n for n, p in sig.parameters.items() if p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD][1:]
    kw = [n for n, p in sig.parameters.items() if p.kind is inspect.Parameter.KEYWORD_ONLY]
    assert pos == ["audio", "lengths", "only_z", "only_mean"] and kw == ["noise"]
    assert sig.parameters["only_z"].default is False and sig.parameters["only_mean"].default is False and sig.parameters["noise"].default is None
    sig = inspect.signature(Vocoder.extract_ragged)
    assert list(sig.parameters) == ["self", "audio", "sample_rate", "lengths", "keyshift", "kwargs"]
    assert sig.parameters["keyshift"].default == 0 and sig.parameters["kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    assert "not in the reference" in Hifi_VAEGAN.extract_ragged.__doc__ and "not in the reference" in Vocoder.extract_ragged.__doc__


def _vocoder():
    from diffusion.vocoder import Vocoder
    from encoder.hifi_vaegan.hifi_vaegan import Hifi_VAEGAN
    from lds import arch
    voc = Vocoder.__new__(Vocoder)
    voc.vocoder = Hifi_VAEGAN(None, device="cpu", h=arch.SYNTHETIC_VOCODER_H, state={}, encoder_state={})
    voc.vocoder_sample_rate, voc.vocoder_hop_size, voc.dimension = 44100, 512, 80
    return voc


@pytest.mark.parametrize("B,lengths", [(3, [1000, 1000]), (3, [1000, 1000, 1000, 1000]), (2, [0, 1000]), (2, [1000, 1001]), (2, [-5, 7]),
                                       (65, [10] * 65)])
def test_extract_ragged_rejects_bad_lengths(B, lengths):
    """a wrong count, a length of 0 (or below), a length beyond the buffer and more than 64 clips are ValueErrors, on any device"""
    import numpy as np
    import torch
    voc = _vocoder()
    audio = torch.zeros(B, 1000)
    for ln in (lengths, tuple(lengths), np.array(lengths), torch.tensor(lengths)):
        with pytest.raises(ValueError, match="lengths|64 clips"):
            voc.extract_ragged(audio, 44100, ln)
        with pytest.raises(ValueError, match="lengths|64 clips"):
            voc.vocoder.extract_ragged(audio, ln, only_z=True)


def test_extract_ragged_checks_like_extract_and_has_no_cpu_fallback():
    import torch
    voc = _vocoder()
    audio = torch.zeros(2, 1024)
    with pytest.raises(ValueError, match="extract_ragged: keyshift"):
        voc.extract_ragged(audio, 44100, [1024, 7], keyshift=1)
    with pytest.raises(ValueError, match="16000.*44100"):
        voc.extract_ragged(audio, 16000, [1024, 7])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        voc.extract_ragged(audio, 44100, [1024, 7])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        voc.vocoder.extract_ragged(audio, [1024, 7], only_z=True)


def test_ragged_encoder_symbols_declared_and_exported():
    from lds import native
    hdr = open(os.path.join(ROOT, "include", "lds.h")).read()
    assert re.search(r"int\s+lds_vae_encoder_forward_ragged\(lds_vae_encoder\* e, const float\* audio, const int32_t\* lengths, const float\* noise,"
                     r"\s+float\* out,\s+float\* z, int only_mean, void\* ws, size_t ws_bytes, int B, int64_t L, void\* stream\);", hdr)
    assert "lds_test_conv_down_ragged(" in open(os.path.join(ROOT, "include", "lds_test.h")).read()
    assert "lds_vae_encoder_forward_ragged" in native.EXPORTS and "lds_test_conv_down_ragged" in native.TEST_EXPORTS
    if not os.path.exists(native.LIB_PATH):
        pytest.skip("liblds.so is not built")
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {"lds_vae_encoder_forward_ragged", "lds_test_conv_down_ragged"} <= syms


DRIVER = r'''
import ctypes as C, sys
sys.path.insert(0, {pkg!r})
from lds import arch, init_weights, native
native.LIB_PATH = {lib!r}
L = native.lib()
h = arch.SYNTHETIC_VOCODER_H
e = native.VaeEncoder(h, init_weights.init_state(arch.encoder_param_shapes(h), 0))
n = 37 * 512
nb = C.c_size_t()
assert L.lds_vae_encoder_workspace_bytes(e.h, 3, C.c_int64(n), C.byref(nb)) == 0
ws = (C.c_char * nb.value)()       # a workspace big enough: every refusal below is about the arguments
dummy = (C.c_float * 8)()
def call(lens, B=3, L_=n, z=None, noise=None):
    arr = (C.c_int32 * max(B, 1))(*lens) if lens is not None else None
    return L.lds_vae_encoder_forward_ragged(e.h, dummy, arr, noise, dummy, z, 0, ws, C.c_size_t(nb.value), B, C.c_int64(L_), None)
assert call(None) == -1 and "lengths is null" in L.lds_last_error().decode()
for lens, bad in (([n, 0, 5], "length[1] = 0"), ([n, 5, n + 1], "length[2] = %d" % (n + 1)), ([-3, 5, 5], "length[0] = -3")):
    assert call(lens) == -1, lens
    msg = L.lds_last_error().decode()
    assert bad in msg and "1 .. %d" % n in msg, msg
assert call([10] * 65, B=65) == -1 and "at most 64" in L.lds_last_error().decode() and "65" in L.lds_last_error().decode()
assert call([10, 10, 10], L_=n + 1) == -1 and "multiple of the hop" in L.lds_last_error().decode()
assert call([10, 10, 10], z=dummy) == -1      # z needs noise
assert L.lds_vae_encoder_forward_ragged(e.h, dummy, (C.c_int32 * 3)(10, 10, 10), None, dummy, None, 0, ws, C.c_size_t(64), 3, C.c_int64(n), None) == -2
assert "workspace too small" in L.lds_last_error().decode()
# the single-op entry refuses null lengths, B > 64 and out-of-range values before anything is uploaded or launched
li = (C.c_int32 * 2)(8, 8)
assert L.lds_test_conv_down_ragged(dummy, dummy, None, 1, 16, 4, 2, 8, 2, C.c_float(0.1), None, li, 0, dummy, None, C.c_size_t(0), None) == -1
assert L.lds_test_conv_down_ragged(dummy, dummy, None, 1, 16, 4, 2, 8, 65, C.c_float(0.1), li, li, 0, dummy, None, C.c_size_t(0), None) == -1
for a, b, bad in (((9, 8), (4, 4), "lengths_in[0] = 9"), ((8, 8), (4, 5), "lengths_out[1] = 5")):
    assert L.lds_test_conv_down_ragged(dummy, dummy, None, 1, 16, 4, 2, 8, 2, C.c_float(0.1), (C.c_int32 * 2)(*a), (C.c_int32 * 2)(*b), 0, dummy, None,
                                       C.c_size_t(0), None) == -1
    assert bad in L.lds_last_error().decode(), L.lds_last_error().decode()
del e
print("ragged encoder driver ok")
'''


def test_ragged_encoder_c_entry_validation_under_asan_ubsan():
    csrc = os.path.join(PKG, "csrc")
    r = subprocess.run(["make", "-C", csrc, "-j", "8", "asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lib = os.path.join(csrc, "build_asan", "liblds_host_asan.so")
    rt = sorted(glob.glob("/opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.asan-x86_64.so"))
    assert rt, "the sanitizer runtime of the ROCm clang is missing"
    env = dict(os.environ, LD_PRELOAD=rt[-1], ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1",
               PYTHONDONTWRITEBYTECODE="1")
    p = subprocess.run([sys.executable, "-c", DRIVER.format(pkg=PKG, lib=lib)], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0 and "ragged encoder driver ok" in p.stdout, (p.returncode, p.stdout[-1500:], p.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr, p.stderr[-4000:]
