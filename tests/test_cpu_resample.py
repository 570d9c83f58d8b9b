"""The polyphase resampler without a GPU: the float64 closed form that is the contract of lds_resample (include/lds.h) against a
restatement of torchaudio's strided-convolution form and against scipy.signal.upfirdn, the library's own bank and offset tables against
float64, the output lengths, the public signatures and symbols, every argument limit of the C entries through the host-only sanitizer
build, and the refusals of the Python surface (Kaiser window, CPU tensors, the rate check that stays the default)."""
import glob
import inspect
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import resample_numpy as RN
from conftest import PKG, ROOT

PAIRS = [(44100, 16000), (16000, 44100), (48000, 16000), (22050, 44100), (44100, 48000), (16000, 16001)]
LENGTHS = [1, 7, 441, 442, 5000]
NAMES = ["lds_resample", "lds_resample_ragged"]


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_closed_form_equals_the_strided_conv_form(pair):
    rng = np.random.default_rng(pair[0] + pair[1])
    for L in LENGTHS:
        x = rng.standard_normal(L)
        a, b = RN.closed_form(x, *pair), RN.conv_form(x, *pair)
        O, N = RN.reduced(*pair)
        assert len(a) == len(b) == math.ceil(N * L / O)
        err = float(np.abs(a - b).max())
        print(f"{pair[0]}->{pair[1]} L {L}: {err:.2e}")
        assert err <= 1e-12, (pair, L, err)


@pytest.mark.parametrize("pair", PAIRS[:5], ids=lambda p: f"{p[0]}to{p[1]}")
def test_closed_form_equals_upfirdn_with_the_prototype_filter(pair):
    """out[m] = (x upsampled by N, filtered by h[k] = g(k / (O N)), every O-th sample): scipy's polyphase routine with the bank in double"""
    from scipy.signal import upfirdn
    O, N = RN.reduced(*pair)
    K = int(math.ceil(RN.support_half(O, N)))
    lead = -(-K // O) * O                                   # centre the prototype on a multiple of O: output m is then sample m + lead / O
    h = np.concatenate([np.zeros(lead - K), RN.g_of(np.arange(-K, K + 1), O, N)])
    rng = np.random.default_rng(2 * pair[0] + pair[1])
    for L in LENGTHS:
        x = rng.standard_normal(L)
        a = RN.closed_form(x, *pair)
        y = upfirdn(h, x, up=N, down=O)[lead // O:]
        y = np.concatenate([y, np.zeros(max(0, len(a) - len(y)))])[:len(a)]
        err = float(np.abs(a - y).max())
        print(f"{pair[0]}->{pair[1]} L {L}: {err:.2e}")
        assert err <= 1e-12, (pair, L, err)


@pytest.mark.parametrize("pair,max_taps", list(zip(PAIRS[:5], (34, 13, 37, 13, 13))) + [((16000, 44101), 13)], ids=lambda v: str(v))
def test_library_tables_against_float64(pair, max_taps):
    from lds import native
    t = native.resample_tables(*pair)
    O, N = RN.reduced(*pair)
    bankT, first = t["bankT"], t["first"]
    assert (t["O"], t["N"]) == (O, N) and t["taps"] <= max_taps
    assert bankT.dtype == np.float32 and bankT.shape == (t["taps"], N) and first.dtype == np.int32 and first.shape == (N,)
    assert native.resample_tables(*pair) is t                                           # built once per parameter set
    i = np.arange(N, dtype=np.int64)
    j = first.astype(np.int64)[None, :] + np.arange(t["taps"], dtype=np.int64)[:, None]
    g = RN.g_of(j * N - i[None, :] * O, O, N)
    assert (np.abs(bankT.astype(np.float64) - g) <= np.spacing(np.abs(g).astype(np.float32)).astype(np.float64)).all()      # within 1 fp32 ulp
    # every column torchaudio's bank has and this one leaves out: j in [-width, width + O) outside [first, first + taps); all phases, or,
    # of the 44,101 (x 16,014 columns), blocks of 256 spread over them with both ends
    width = math.ceil(6 * O / (0.99 * min(O, N)))
    starts = range(0, N, 256) if N <= 4096 else sorted({0, N - 256, *range(0, N - 256, 256 * 23)})
    for i0 in starts:
        ii = np.arange(i0, min(N, i0 + 256), dtype=np.int64)
        jj = np.arange(-width, width + O, dtype=np.int64)[:, None]
        out = (jj < first[ii][None, :]) | (jj >= first[ii][None, :] + t["taps"])
        assert (np.abs(RN.g_of(jj * N - ii[None, :] * O, O, N))[out] < 1e-30).all()


def test_output_lengths():
    from lds import native
    for orig, new in PAIRS:
        O, N = RN.reduced(orig, new)
        for q in (1, 3, 100):
            assert native.resample_out_length(q * O, O, N) == q * N == len(RN.closed_form(np.ones(q * O), orig, new)) if q * O <= 1000 else True
            assert native.resample_out_length(q * O + 1, O, N) == q * N + math.ceil(N / O)
            assert native.resample_out_length(q * O - 1, O, N) == q * N - N // O
    assert native.resample_out_length(1323000, 441, 160) == 480000 and native.resample_out_length(0, 441, 160) == 0


def test_signatures_symbols_and_flags():
    from diffusion.vocoder import Vocoder
    from lds import native
    from tools.infer_tools import DiffusionSVC
    from tools.tools import Resample, Units_Encoder
    sig = inspect.signature(Resample.__init__)
    assert [(n, p.default) for n, p in list(sig.parameters.items())[1:]] == [
        ("orig_freq", 16000), ("new_freq", 16000), ("resampling_method", "sinc_interp_hann"), ("lowpass_filter_width", 6), ("rolloff", 0.99)]
    assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for p in sig.parameters.values())
    assert list(inspect.signature(Resample.forward).parameters) == ["self", "waveform"]
    assert list(inspect.signature(Resample.forward_ragged).parameters) == ["self", "waveform", "lengths"]
    assert "not in the reference" in Resample.forward_ragged.__doc__
    import torch
    assert issubclass(Resample, torch.nn.Module) and isinstance(Resample(44100, 16000).to("cpu"), Resample)
    for fn in (Units_Encoder.__init__, DiffusionSVC.load_model):
        p = inspect.signature(fn).parameters["resample"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    # Vocoder's constructor keeps the reference's parameters exactly; its flag is an attribute, False also without __init__
    assert Vocoder.resample is False and Vocoder.__new__(Vocoder).resample is False
    hdr = open(os.path.join(ROOT, "include", "lds.h")).read()
    for n in NAMES:
        assert re.search(r"\b" + n + r"\(", hdr), n
    assert "tools/tools.py:78-84" in hdr and "diffusion/vocoder.py:24-27" in hdr and "semantic_extract.py:49-68" in hdr      # the calls replaced
    assert set(NAMES) <= set(native.EXPORTS)
    assert native.SIGNATURES["lds_resample"] == "i:ppppiiiiqqp" and native.SIGNATURES["lds_resample_ragged"] == "i:ppppppiiiiqqp"
    assert os.path.exists(native.LIB_PATH), "liblds.so is not built"
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(NAMES) <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_refusals_and_the_default_rate_check():
    import torch
    from diffusion.vocoder import Vocoder
    from lds import arch, native
    from tools.tools import Resample, Units_Encoder, WhisperLargeV3
    from encoder.whisper.model import ModelDimensions
    with pytest.raises(NotImplementedError, match="sinc_interp_kaiser"):
        Resample(44100, 16000, "sinc_interp_kaiser")
    with pytest.raises(ValueError, match="Invalid resampling method"):
        Resample(44100, 16000, "linear")
    for bad in (dict(lowpass_filter_width=0), dict(lowpass_filter_width=2.5), dict(rolloff=0.0), dict(rolloff=1.5)):
        with pytest.raises(ValueError, match="lowpass_filter_width|rolloff"):
            Resample(44100, 16000, **bad)
    with pytest.raises(ValueError, match="384000"):
        Resample(400000, 16000)
    with pytest.raises(ValueError, match="taps"):
        Resample(44100, 100)      # 441:1 behind the default filter: 5347 taps
    x = torch.zeros(2, 1000)
    rs = Resample(44100, 16000)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rs(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rs.forward_ragged(x, [1000, 10])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        native.resample(x, native.resample_tables(44100, 16000))
    assert Resample(16000, 16000)(x) is x      # equal rates: the input itself, on any device
    # the default path keeps the rate error; the opt-in path gets as far as the device check
    dims = ModelDimensions(**dict(arch.WHISPER_LARGE_V3_DIMS, n_audio_state=128, n_audio_head=2, n_audio_layer=1))
    model = WhisperLargeV3.synthetic(dims, device="cpu")
    off = Units_Encoder("whisper_large_v3", device="cpu", model=model)
    on = Units_Encoder("whisper_large_v3", device="cpu", model=model, resample=True)
    assert off.resample is False and on.resample is True
    for call in (lambda ue: ue.encode(x[:1], 44100), lambda ue: ue.encode_ragged(x, [1000, 500], 44100),
                 lambda ue: ue.encode_tokens(x[:1], 44100, None), lambda ue: ue.encode_tokens_ragged(x, [1000, 500], None, -1, 44100)):
        with pytest.raises(ValueError, match="44100.*16000.*resample=True / use tools.tools.Resample"):
            call(off)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(on)
    voc = Vocoder.__new__(Vocoder)
    voc.vocoder_sample_rate = 44100
    for call in (lambda: voc.extract(x, 22050), lambda: voc.extract_ragged(x, 22050, [1000, 500])):
        with pytest.raises(ValueError, match="22050.*44100.*resample=True / use tools.tools.Resample"):
            call()
        voc.resample = True
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
        voc.resample = False


DRIVER = r'''
import ctypes as C, sys
sys.path.insert(0, {pkg!r})
from lds import native
native.LIB_PATH = {lib!r}
L = native.lib()
def err():
    return L.lds_last_error().decode()
d = (C.c_float * 64)()      # never touched: every refusal below comes before anything is read or enqueued
i32 = (C.c_int32 * 64)()
lens = (C.c_int32 * 65)(*([100] * 65))
new = (C.c_int64 * 65)()
A = lambda **k: dict(dict(x=d, y=d, bank=d, first=i32, O=441, N=160, taps=34, B=2, L=1000, M=363, ln=lens, new=new), **k)
def dense(a):
    return L.lds_resample(a["x"], a["y"], a["bank"], a["first"], a["O"], a["N"], a["taps"], a["B"], a["L"], a["M"], None)
def ragged(a):
    return L.lds_resample_ragged(a["x"], a["ln"], a["y"], a["new"], a["bank"], a["first"], a["O"], a["N"], a["taps"], a["B"], a["L"], a["M"], None)
for fn in (dense, ragged):
    for k, bad in ((dict(O=0), "O 0"), (dict(O=384001), "O 384001"), (dict(N=0), "N 0"), (dict(N=-3), "N -3"), (dict(N=384001), "N 384001"),
                   (dict(taps=0), "taps 0"), (dict(taps=1025), "taps 1025"), (dict(N=384000, taps=44), "bank of 16896000"),
                   (dict(L=0), "L 0"), (dict(L=-1), "L -1"), (dict(L=(1 << 30) + 1), "L 1073741825"), (dict(B=0), "B 0"), (dict(B=-1), "B -1")):
        assert fn(A(**k)) == -1 and bad in err(), (fn.__name__, k, err())
    for k in (dict(x=None), dict(y=None), dict(bank=None), dict(first=None)):
        assert fn(A(**k)) == -1 and "null" in err(), (fn.__name__, k, err())
assert dense(A(B=65536)) == -1 and "B 65536" in err()
assert dense(A(M=362)) == -1 and dense(A(M=364)) == -1 and "exactly 363" in err()
assert dense(A(O=1, N=384000, L=1 << 30, M=1)) == -1 and "output samples per clip" in err()
assert ragged(A(B=65)) == -1 and "1 .. 64" in err()
assert ragged(A(ln=None)) == -1 and "null lengths" in err()
assert ragged(A(ln=(C.c_int32 * 2)(100, 1001))) == -1 and "lengths[1] = 1001" in err()
assert ragged(A(ln=(C.c_int32 * 2)(-1, 100))) == -1 and "lengths[0] = -1" in err()
assert ragged(A(M=36)) == -1 and "at least 37" in err()      # ceil(160 * 100 / 441) = 37
assert ragged(A(M=0, ln=(C.c_int32 * 2)(0, 0))) == -1
assert ragged(A(M=1 << 31)) == -1
assert new[0] == 0      # a refused call returns no lengths
print("resample driver ok")
'''


def test_resample_c_entry_validation_under_asan_ubsan():
    csrc = os.path.join(PKG, "csrc")
    r = subprocess.run(["make", "-C", csrc, "-j", "8", "asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lib = os.path.join(csrc, "build_asan", "liblds_host_asan.so")
    rt = sorted(glob.glob("/opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.asan-x86_64.so"))
    assert rt, "the sanitizer runtime of the ROCm clang is missing"
    env = dict(os.environ, LD_PRELOAD=rt[-1], ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1",
               PYTHONDONTWRITEBYTECODE="1")
    p = subprocess.run([sys.executable, "-c", DRIVER.format(pkg=PKG, lib=lib)], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0 and "resample driver ok" in p.stdout, (p.returncode, p.stdout[-1500:], p.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr, p.stderr[-4000:]
