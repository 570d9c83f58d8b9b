"""The VAE encoder without a GPU: parameter shapes against the reference manifest, the module API (signatures, the two documented
deviations of Vocoder.extract, no CPU fallback), and the host side of lds_vae_encoder_* (weight-norm folding, weight upload, workspace
planning, argument validation) under AddressSanitizer + UBSan, as tests/test_cpu_sanitizer.py does for the other handles."""
import glob
import inspect
import json
import os
import subprocess
import sys

import pytest

from conftest import GOLDEN, PKG, ROOT

H_RB2 = dict(resblock="2", resblock_dilation_sizes=[[1, 3], [1, 3], [1, 3]])


def test_encoder_param_shapes_match_reference_manifest():
    from lds import arch
    got = {k: list(v) for k, v in arch.encoder_param_shapes(arch.SYNTHETIC_VOCODER_H).items()}
    ref = json.load(open(os.path.join(GOLDEN, "manifest_encoder.json")))
    assert list(got) == list(ref) and got == ref


def test_encoder_param_shapes_resblock2_match_fixture():
    import numpy as np
    from lds import arch
    g = np.load(os.path.join(GOLDEN, "encoder_rb2.npz"))
    h = json.loads(bytes(g["h_json"]).decode())
    assert h == dict(arch.SYNTHETIC_VOCODER_H, **H_RB2)
    sh = arch.encoder_param_shapes(h)
    assert "resblocks.14.convs.1.weight_v" in sh and not any("convs1" in k for k in sh)
    assert sh["resblocks.14.convs.1.weight_v"] == (512, 512, 11) and sh["resblocks.0.convs.0.weight_v"] == (32, 32, 3)
    assert sh["ups.4.weight_g"] == (512, 1, 1) and sh["conv_post.weight_v"] == (160, 512, 7)


def test_extract_signatures():
    from diffusion.vocoder import Vocoder
    from encoder.hifi_vaegan.hifi_vaegan import Hifi_VAEGAN

    def split(f):
        sig = inspect.signature(f)
        kw = [p for p in sig.parameters.values() if p.kind is inspect.Parameter.KEYWORD_ONLY]
        assert all(p.default is None for p in kw)
        return [n for n, p in sig.parameters.items() if p.kind not in (inspect.Parameter.KEYWORD_ONLY, inspect.Parameter.VAR_KEYWORD)][1:], \
            [p.name for p in kw]
    assert split(Hifi_VAEGAN.extract) == (["audio", "only_z", "only_mean"], ["noise"])
    assert split(Hifi_VAEGAN.__init__)[1] == ["encoder_state"]
    assert split(Vocoder.extract) == (["audio", "sample_rate", "keyshift"], [])
    assert inspect.signature(Vocoder.extract).parameters["keyshift"].default == 0


def _vocoder():
    from diffusion.vocoder import Vocoder
    from encoder.hifi_vaegan.hifi_vaegan import Hifi_VAEGAN
    from lds import arch
    voc = Vocoder.__new__(Vocoder)
    voc.vocoder = Hifi_VAEGAN(None, device="cpu", h=arch.SYNTHETIC_VOCODER_H, state={}, encoder_state={})
    voc.vocoder_sample_rate, voc.vocoder_hop_size, voc.dimension = 44100, 512, 80
    return voc


def test_vocoder_extract_deviations_and_no_cpu_fallback():
    import torch
    voc = _vocoder()
    audio = torch.zeros(1, 1024)
    with pytest.raises(ValueError, match="keyshift"):
        voc.extract(audio, 44100, keyshift=1)
    with pytest.raises(ValueError, match="16000.*44100"):
        voc.extract(audio, 16000)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        voc.extract(audio, 44100)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        voc.vocoder.extract(audio, only_z=True)


def test_vae_encoder_rejects_a_hop_size_that_is_not_the_downsampling():
    """extract pads to hop_size, the handle needs multiples of prod(upsample_rates): a config where they differ fails when the encoder is
    built, with both numbers, before the library is asked anything"""
    from lds import arch, native
    with pytest.raises(ValueError, match="hop_size 256 != prod\\(upsample_rates\\) 512"):
        native.VaeEncoder(dict(arch.SYNTHETIC_VOCODER_H, hop_size=256), {})


DRIVER = r'''
import ctypes as C, sys
sys.path.insert(0, {pkg!r})
from lds import arch, init_weights, native
native.LIB_PATH = {lib!r}
L = native.lib()
nb = C.c_size_t()
for h in (arch.SYNTHETIC_VOCODER_H, dict(arch.SYNTHETIC_VOCODER_H, resblock="2", resblock_dilation_sizes=[[1, 3], [1, 3], [1, 3]])):
    st = init_weights.init_state(arch.encoder_param_shapes(h), 0)
    e = native.VaeEncoder(h, st)                      # weight-norm folding + upload of 291 / 201 tensors
    sizes = []
    for (B, L_) in ((16, 512 * 512), (1, 12 * 512), (3, 37 * 512)):
        sizes.append(e.workspace_bytes(B, L_))
    assert sizes[0] > sizes[2] > sizes[1] > 0, sizes
    # workspace of 16 x 512 frames: the 16-channel front end at full rate dominates (five ping-pong tensors) + the K4P tensors
    assert sizes[0] >= 5 * 16 * 16 * 512 * 512 * 4, sizes[0]
    # folded weights are accepted too (already remove_weight_norm'ed checkpoints)
    fold = {{}}
    import numpy as np
    for k, v in st.items():
        if k.endswith("weight_v"):
            g = st[k[:-1] + "g"]
            fold[k[:-2]] = (v * (g / np.sqrt((v.astype(np.float64) ** 2).sum(axis=(1, 2), keepdims=True)))).astype(np.float32)
        elif not k.endswith("weight_g"):
            fold[k] = v
    native.VaeEncoder(h, fold)
    del e
h = arch.SYNTHETIC_VOCODER_H
st = init_weights.init_state(arch.encoder_param_shapes(h), 0)
e = native.VaeEncoder(h, st)
# rejection paths: every one before anything is enqueued
for B, L_ in ((0, 512), (-1, 512), (1, 0), (1, 513), (2, 12 * 512 - 100)):
    assert L.lds_vae_encoder_workspace_bytes(e.h, B, C.c_int64(L_), C.byref(nb)) == -1, (B, L_)
    assert "multiple of the hop" in L.lds_last_error().decode()
dummy = (C.c_float * 8)()
ws = (C.c_char * 64)()
for B, L_ in ((0, 512), (1, 513)):
    assert L.lds_vae_encoder_forward(e.h, dummy, None, dummy, None, 0, ws, C.c_size_t(64), B, C.c_int64(L_), None) == -1
assert L.lds_vae_encoder_forward(e.h, dummy, None, dummy, dummy, 0, ws, C.c_size_t(64), 1, C.c_int64(512), None) == -1      # z needs noise
assert L.lds_vae_encoder_forward(e.h, dummy, None, dummy, None, 0, ws, C.c_size_t(64), 1, C.c_int64(512), None) == -2      # workspace too small
assert "workspace too small" in L.lds_last_error().decode()
for bad in (dict(h, upsample_kernel_sizes=[16, 16, 4, 4, 6]), dict(h, upsample_rates=[8, 8, 2, 2, 3], upsample_kernel_sizes=[16, 16, 4, 4, 6]),
            dict(h, upsample_rates=[32, 2, 2, 2, 2], upsample_kernel_sizes=[64, 4, 4, 4, 4])):
    bad["hop_size"] = int(np.prod(bad["upsample_rates"]))      # (a consistent hop: the geometry itself is what the library refuses)
    try:
        native.VaeEncoder(bad, st); raise SystemExit("accepted an unsupported geometry")
    except RuntimeError as ex:
        assert "unsupported downsample geometry" in str(ex), ex
part = dict(st); del part["resblocks.7.convs2.1.weight_v"]
try:
    native.VaeEncoder(h, part); raise SystemExit("accepted a missing key")
except RuntimeError as ex:
    assert "error -4" in str(ex) and "resblocks.7.convs2.1.weight_v" in str(ex), ex
wrong = dict(st); wrong["ups.3.weight_v"] = st["ups.3.weight_v"][:, :64]
try:
    native.VaeEncoder(h, wrong); raise SystemExit("accepted a wrongly shaped tensor")
except RuntimeError as ex:
    assert "ups.3.weight_v (wrong size)" in str(ex), ex
del e
print("encoder sanitizer driver ok")
'''


def test_encoder_host_side_under_asan_ubsan():
    csrc = os.path.join(PKG, "csrc")
    r = subprocess.run(["make", "-C", csrc, "-j", "8", "asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lib = os.path.join(csrc, "build_asan", "liblds_host_asan.so")
    rt = sorted(glob.glob("/opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.asan-x86_64.so"))
    assert rt, "the sanitizer runtime of the ROCm clang is missing"
    env = dict(os.environ, LD_PRELOAD=rt[-1], ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1",
               PYTHONDONTWRITEBYTECODE="1")
    p = subprocess.run([sys.executable, "-c", DRIVER.format(pkg=PKG, lib=lib)], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0 and "encoder sanitizer driver ok" in p.stdout, (p.returncode, p.stdout[-1500:], p.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr, p.stderr[-4000:]
