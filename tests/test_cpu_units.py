"""The Whisper units encoder (tools.tools.Units_Encoder / WhisperLargeV3, include/lds.h lds_whisper_*) without a GPU: the computed mel
filter bank, the numpy restatement the GPU tests lean on (pinned to the fixtures recorded from the reference), the parameter enumeration and
public signatures, the exported symbols, the Python argument validation, and the C entries' argument validation on the sanitizer build of
the host side (make asan), where nothing can be launched: every refusal must come before anything is enqueued."""
import glob
import inspect
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import whisper_numpy as wnp
from conftest import GOLDEN, PKG, ROOT


def _filters(n_mels):
    return np.load(os.path.join(GOLDEN, "whisper_mel_filters.npz"))[f"mel_{n_mels}"]


@pytest.mark.parametrize("n_mels", [80, 128])
def test_computed_mel_filters_equal_the_reference_bank(n_mels):
    """2e-8 absolute on a bank whose peak is 0.042: the reference's file is librosa's float32 output, the package computes the same
    formula in float64 and rounds once (a float32 evaluation of the ramps differs from it by a few 1e-9)"""
    from lds import arch
    ref = _filters(n_mels)
    got = arch.whisper_mel_filters(n_mels)
    assert got.dtype == np.float32 and got.shape == ref.shape == (n_mels, 201)
    assert np.abs(got.astype(np.float64) - ref).max() <= 2e-8
    assert (got >= 0).all() and np.count_nonzero(got) == np.count_nonzero(ref)


@pytest.mark.parametrize("n_mels", [80, 128])
def test_numpy_log_mel_reproduces_the_reference(n_mels):
    """float64 mode: the fixture holds the reference's lines evaluated in float64, stored rounded to float32 (values below 2: half an ulp
    is 6e-8), so 1e-7.  float32 mode: the restatement is one more fp32 evaluation of the same operator, so its distance from the float64
    result is bounded by twice the reference's own worst fp32 error over the clips (per clip E_ref spans 5e-7 .. 4e-5 with the clip
    length; a two-frame clip's E_ref is below what any fp32 400-term sum guarantees)"""
    from lds import init_weights
    z = np.load(os.path.join(GOLDEN, f"whisper_logmel_{n_mels}.npz"))
    filt = _filters(n_mels)
    worst = max(float(z[f"eref_{i}"]) for i in range(5))
    for i in range(5):
        n = int(z[f"n_{i}"])
        audio = wnp.make_signal(f"clip{i}", n, int(z[f"seed_{i}"]), init_weights.uniform, bool(z[f"quiet_{i}"]))
        ref = z[f"ref64_{i}"].astype(np.float64)
        assert ref.shape == (n_mels, n // 160)
        m64 = wnp.log_mel(audio, filt, np.float64)
        m32 = wnp.log_mel(audio, filt, np.float32)
        assert m32.dtype == np.float32 and m32.shape == ref.shape
        e64, e32 = np.abs(m64 - ref).max(), np.abs(m32 - ref).max()
        print(f"clip {i} ({n} samples): fp64 {e64:.2e}, fp32 {e32:.2e}, E_ref {float(z[f'eref_{i}']):.2e}")
        assert e64 <= 1e-7, (i, e64)
        assert e32 <= 2 * worst, (i, e32, worst)


def test_numpy_encoder_reproduces_the_reference():
    """2e-5 x absmax, the project's bound for an fp32 forward against the reference (the GPU tests' bound); the float64 mode sits at the
    reference's own fp32-vs-fp64 gap"""
    from lds import arch, init_weights
    z = np.load(os.path.join(GOLDEN, "whisper_encoder.npz"))
    for name in "ab":
        n_mels, C, H, layers, F, seed = (int(v) for v in z[name + "_dims"])
        w = arch.whisper_init_state(n_mels, C, layers, 0)
        mel = init_weights.uniform(f"fix.whisper.{name}.mel", (1, n_mels, F), seed, -1.0, 1.5)
        ref = z[name + "_out"][0]
        assert ref.shape == ((F - 1) // 2 + 1, C)
        for dt in (np.float32, np.float64):
            got = wnp.encoder(w, mel[0], H, dt)
            err = np.abs(got - ref).max() / np.abs(ref).max()
            print(name, dt.__name__, err, float(z[name + "_gap"]))
            assert err <= 2e-5, (name, dt, err)
    w = arch.whisper_init_state(128, 128, 4, 0)
    audio = wnp.make_signal("e2e", int(z["e2e_n"]), int(z["e2e_seed"]), init_weights.uniform, False)
    for dt in (np.float32, np.float64):
        got = wnp.encode(w, audio, _filters(128), 2, dt)
        err = np.abs(got - z["e2e_out"]).max() / np.abs(z["e2e_out"]).max()
        print("e2e", dt.__name__, err, float(z["e2e_gap"]))
        assert err <= 2e-5, (dt, err)


def test_param_shapes_equal_the_reference_manifest():
    from encoder.whisper.model import ModelDimensions, Whisper
    from lds import arch
    man = json.load(open(os.path.join(GOLDEN, "manifest_whisper.json")))
    assert man["large_v3_dims"] == arch.WHISPER_LARGE_V3_DIMS
    for key in ("large_v3", "small"):
        d = man[key + "_dims"]
        got = arch.whisper_param_shapes(d["n_mels"], d["n_audio_state"], d["n_audio_layer"])
        assert list(got.keys()) == list(man[key].keys())
        assert {k: list(v) for k, v in got.items()} == man[key]
    small = Whisper(ModelDimensions(**man["small_dims"]))
    assert {k: list(v.shape) for k, v in small.state_dict().items()} == man["small"]
    assert [f.name for f in ModelDimensions.__dataclass_fields__.values()] == list(man["large_v3_dims"].keys())


def _params(sig):
    return [(n, p.default) for n, p in sig.parameters.items() if p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]


def _ref_params(text):
    """'(self, a, b=1)' as recorded from the reference -> [(name, default)]"""
    ns = {}
    exec(f"def f{text}: pass", ns)
    return _params(inspect.signature(ns["f"]))


def test_public_signatures_equal_the_reference():
    from encoder.whisper import audio as wa
    from tools.tools import Units_Encoder, WhisperLargeV3
    sig = json.load(open(os.path.join(GOLDEN, "manifest_whisper.json")))["signatures"]
    # the same positional parameters, names, order and defaults; extensions are keyword-only
    assert _params(inspect.signature(Units_Encoder.__init__)) == _ref_params(sig["Units_Encoder.__init__"])
    assert str(inspect.signature(Units_Encoder.encode)) == sig["Units_Encoder.encode"]
    assert str(inspect.signature(WhisperLargeV3.__call__)) == sig["WhisperLargeV3.__call__"]
    ref_init = _ref_params(sig["WhisperLargeV3.__init__"])
    got_init = _params(inspect.signature(WhisperLargeV3.__init__))
    assert got_init[:len(ref_init)] == ref_init and got_init[len(ref_init):] == [("checkpoint", "pretrain/large-v3_encoder.pt")]
    assert [n for n, _ in _params(inspect.signature(wa.log_mel_spectrogram))] == re.findall(r"(\w+): ", sig["log_mel_spectrogram"])      # (all four are annotated)
    assert [d for _, d in _params(inspect.signature(wa.log_mel_spectrogram))][1:] == [128, 0, None]
    assert list(inspect.signature(wa.mel_filters.__wrapped__).parameters) == ["device", "n_mels"]
    assert list(inspect.signature(Units_Encoder.encode_ragged).parameters)[:3] == ["self", "audio", "lengths"]
    assert "not in the reference" in Units_Encoder.encode_ragged.__doc__
    assert (wa.SAMPLE_RATE, wa.N_FFT, wa.HOP_LENGTH, wa.N_SAMPLES) == (16000, 400, 160, 480000)


def test_whisper_symbols_declared_and_exported():
    from lds import native
    hdr = open(os.path.join(ROOT, "include", "lds.h")).read()
    names = ["lds_whisper_create", "lds_whisper_destroy", "lds_whisper_workspace_bytes", "lds_whisper_logmel", "lds_whisper_encode_mel", "lds_whisper_encode"]
    for n in names:
        assert re.search(r"\b" + n + r"\(", hdr), n
    assert re.search(r"typedef struct \{ int n_mels, n_state, n_head, n_layer, n_ctx; \} lds_whisper_cfg;", hdr)
    assert set(names) <= set(native.EXPORTS)
    if not os.path.exists(native.LIB_PATH):
        pytest.skip("liblds.so is not built")
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(names) <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def _synthetic_encoder():
    """a Units_Encoder over a handle-less WhisperLargeV3: argument checks come before the native handle is built"""
    from encoder.whisper.model import ModelDimensions
    from lds import arch
    from tools.tools import Units_Encoder, WhisperLargeV3
    dims = ModelDimensions(**dict(arch.WHISPER_LARGE_V3_DIMS, n_audio_state=128, n_audio_head=2, n_audio_layer=1))
    return Units_Encoder("whisper_large_v3", device="cpu", model=WhisperLargeV3.synthetic(dims, device="cpu"))


def test_unbuilt_cases_and_cpu_tensors_raise():
    import torch
    from tools.infer_tools import DiffusionSVC
    from tools.tools import Units_Encoder
    with pytest.raises(NotImplementedError, match="transformers"):
        Units_Encoder("w2v-bert")
    with pytest.raises(NotImplementedError, match="fairseq"):
        Units_Encoder("xlsr_53_56k")
    with pytest.raises(ValueError, match="Unknown units encoder"):
        Units_Encoder("contentvec")
    with pytest.raises(NotImplementedError, match="rfa441to512"):
        Units_Encoder("whisper_large_v3", units_forced_mode="rfa441to512")
    ue = _synthetic_encoder()
    audio = torch.zeros(1, 16000)
    with pytest.raises(ValueError, match="44100.*16000"):
        ue.encode(audio, 44100)
    with pytest.raises(ValueError, match="44100.*16000"):
        ue.encode_ragged(audio, [16000], 44100)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ue.encode(audio, 16000)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ue.encode_ragged(audio, [16000])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ue.model(audio)
    from encoder.whisper.audio import log_mel_spectrogram
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        log_mel_spectrogram(audio[0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ue.model.model.encoder(torch.zeros(1, 128, 100))
    svc = DiffusionSVC(device="cpu")
    with pytest.raises(NotImplementedError, match="units_encoder_checkpoint"):
        svc.encode_units(audio, 16000)
    svc.units_encoder = ue
    with pytest.raises(ValueError, match="44100.*16000"):
        svc.encode_units(audio)


DRIVER = r'''
import ctypes as C, sys
sys.path.insert(0, {pkg!r})
import numpy as np
from lds import arch, native
native.LIB_PATH = {lib!r}
L = native.lib()
def err():
    return L.lds_last_error().decode()
filt = arch.whisper_mel_filters(128)
state = arch.whisper_init_state(128, 128, 2, 0)
def create(n_mels=128, n_state=128, n_head=2, n_layer=2, n_ctx=1500, st=state):
    c = native.WhisperCfg(n_mels, n_state, n_head, n_layer, n_ctx)
    n, names, ptrs, numel, keep = native._host_tensor_table(st)
    h = C.c_void_p()
    return L.lds_whisper_create(C.byref(c), n, names, ptrs, numel, C.c_void_p(filt.ctypes.data), C.byref(h)), h
for kw, bad in ((dict(n_mels=96), "n_mels 96"), (dict(n_state=96, n_head=2), "multiple of 64"), (dict(n_head=4), "must be 64"), (dict(n_layer=0), "n_layer 0"),
                (dict(n_ctx=0), "n_ctx 0")):
    rc, h = create(**kw)
    assert rc == -1 and bad in err(), (kw, rc, err())
rc, h = create(st={{k: v for k, v in state.items() if k != "encoder.blocks.1.attn.key.weight"}})
assert rc == -4 and "encoder.blocks.1.attn.key.weight" in err(), (rc, err())
rc, h = create(st=dict(state, **{{"encoder.blocks.0.attn.key.bias": np.zeros(128, np.float32)}}))      # an extra tensor is ignored
assert rc == 0
L.lds_whisper_destroy(h)
w = native.Whisper(128, 128, 2, 2, 1500, state, filt)      # packs LayerNorm folds, the sinusoid table, the DFT basis
n = 480000
nb = C.c_size_t()
assert L.lds_whisper_workspace_bytes(w.h, 3, C.c_int64(n), C.byref(nb)) == 0 and nb.value > 0
assert L.lds_whisper_workspace_bytes(w.h, 0, C.c_int64(n), C.byref(nb)) == -1 and "B 0" in err()
assert L.lds_whisper_workspace_bytes(w.h, 1, C.c_int64(399), C.byref(nb)) == -1 and "400" in err()
assert L.lds_whisper_workspace_bytes(w.h, 1, C.c_int64(n + 320), C.byref(nb)) == -1 and "n_ctx 1500" in err()
assert L.lds_whisper_workspace_bytes(w.h, 3, C.c_int64(n), C.byref(nb)) == 0
ws = (C.c_char * 4096)()      # never touched: every refusal below comes before the workspace is laid out
dummy = (C.c_float * 8)()
big = C.c_size_t(nb.value)
def calls(lens, B=3, L_=n):
    arr = (C.c_int32 * max(B, 1))(*lens) if lens is not None else None
    return [L.lds_whisper_encode(w.h, dummy, arr, dummy, ws, big, B, C.c_int64(L_), None),
            L.lds_whisper_logmel(w.h, dummy, arr, dummy, ws, big, B, C.c_int64(L_), None)]
for lens, bad in (([n, 399, 5000], "length[1] = 399"), ([n, 5000, n + 1], "length[2] = %d" % (n + 1)), ([-3, 5000, 5000], "length[0] = -3")):
    for rc in calls(lens):
        assert rc == -1 and bad in err() and "400 .. %d" % n in err(), (lens, rc, err())
for rc in calls([400] * 65, B=65):
    assert rc == -1 and "at most 64" in err()
for rc in calls(None, B=0):
    assert rc == -1 and "B 0" in err()
for rc in calls(None, L_=399):
    assert rc == -1 and "400" in err()
for rc in calls(None, L_=n + 320):
    assert rc == -1 and "n_ctx 1500" in err()
assert L.lds_whisper_encode(w.h, None, None, dummy, ws, big, 3, C.c_int64(n), None) == -1
assert L.lds_whisper_encode(w.h, dummy, None, None, ws, big, 3, C.c_int64(n), None) == -1
assert L.lds_whisper_encode(None, dummy, None, dummy, ws, big, 3, C.c_int64(n), None) == -1
F = n // 160
for nf, bad in (([F, 0, 5], "n_frames[1] = 0"), ([F, 5, F + 1], "n_frames[2] = %d" % (F + 1))):
    assert L.lds_whisper_encode_mel(w.h, dummy, (C.c_int32 * 3)(*nf), dummy, ws, big, 3, F, None) == -1 and bad in err(), err()
assert L.lds_whisper_encode_mel(w.h, dummy, None, dummy, ws, big, 3, 0, None) == -1
assert L.lds_whisper_encode_mel(w.h, dummy, None, dummy, ws, big, 3, F + 2, None) == -1 and "n_ctx 1500" in err()
assert L.lds_whisper_encode_mel(w.h, dummy, (C.c_int32 * 65)(*([5] * 65)), dummy, ws, big, 65, F, None) == -1 and "at most 64" in err()
# a workspace that is too small is refused with the size that is needed, before anything is enqueued
small = C.c_size_t(4096)
lens3 = (C.c_int32 * 3)(n, 5000, 400)
assert L.lds_whisper_encode(w.h, dummy, lens3, dummy, ws, small, 3, C.c_int64(n), None) == -2 and "workspace too small" in err()
assert L.lds_whisper_logmel(w.h, dummy, None, dummy, ws, small, 3, C.c_int64(n), None) == -2
assert L.lds_whisper_encode_mel(w.h, dummy, None, dummy, ws, small, 3, F, None) == -2
# the Python layer refuses the same before it reaches the library
for fn, a in ((w._check, (0, n)), (w._check, (1, 399)), (w._check, (1, n + 320)), (w.lengths, ([400] * 65, 65, n)), (w.lengths, ([399, 400], 2, n)),
              (w.lengths, ([400, n + 1], 2, n)), (w.lengths, ([400], 2, n))):
    try:
        fn(*a); raise SystemExit("accepted %r" % (a,))
    except ValueError:
        pass
for kw in (dict(n_mels=96), dict(n_state=96), dict(n_head=3), dict(n_layer=0)):
    a = dict(n_mels=128, n_state=128, n_head=2, n_layer=2); a.update(kw)
    try:
        native.Whisper(a["n_mels"], a["n_state"], a["n_head"], a["n_layer"], 1500, state, filt); raise SystemExit("accepted %r" % (kw,))
    except ValueError:
        pass
del w
print("whisper driver ok")
'''


def test_whisper_c_entry_validation_under_asan_ubsan():
    csrc = os.path.join(PKG, "csrc")
    r = subprocess.run(["make", "-C", csrc, "-j", "8", "asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lib = os.path.join(csrc, "build_asan", "liblds_host_asan.so")
    rt = sorted(glob.glob("/opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.asan-x86_64.so"))
    assert rt, "the sanitizer runtime of the ROCm clang is missing"
    env = dict(os.environ, LD_PRELOAD=rt[-1], ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1",
               PYTHONDONTWRITEBYTECODE="1")
    p = subprocess.run([sys.executable, "-c", DRIVER.format(pkg=PKG, lib=lib)], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0 and "whisper driver ok" in p.stdout, (p.returncode, p.stdout[-1500:], p.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr, p.stderr[-4000:]
