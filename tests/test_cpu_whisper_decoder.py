"""Whisper's text decoder without a GPU: the numpy restatement the GPU tests lean on (pinned to the fixtures recorded from the reference's
blocks), the parameter enumeration against the recorded manifest, the unchanged default `Whisper(dims)`, the binding's mirrors of the C
structs, the special-token table, the tool's argument parser, and the host side of the C entries -- create, plans and every refusal -- as a
stand-alone program under AddressSanitizer + UBSan, where nothing can be launched."""
import ctypes as C
import importlib.util
import json
import os
import re
import subprocess

import numpy as np
import pytest

import whisper_decoder_numpy as dnp
from conftest import GOLDEN, PKG, ROOT

MANIFEST = json.load(open(os.path.join(GOLDEN, "manifest_whisper_decoder.json")))


def _fix():
    return dict(np.load(os.path.join(GOLDEN, "whisper_decoder.npz")))


def _state(name, z):
    from lds import arch
    c = dnp.CONFIGS[name]
    return arch.whisper_decoder_init_state(c["n_vocab"], c["n_text_ctx"], c["n_state"], c["n_layer"], int(z[f"seed_{name}"]))


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_numpy_restatement_reproduces_the_fixtures(name):
    """float64 against float64 (the reference's blocks with its two .float() calls lifted): 1e-9 x absmax on the teacher-forced logits,
    identical greedy ids, log-probs to 1e-9 x absmax.  The float32 mode stays within 4 x the oracle's own fp32-against-fp64 gap."""
    from lds import init_weights
    z = _fix()
    c = dnp.CONFIGS[name]
    w = _state(name, z)
    inp = dnp.inputs(name, init_weights.uniform, int(z[f"seed_{name}"]))
    ref = z[f"logits_{name}"]
    got = dnp.logits_batch(w, c, inp["tf_tokens"], inp["units"], dnp.N_FRAMES, dnp.TF_LEN)
    absmax = np.abs(ref).max()
    assert np.abs(got - ref).max() <= 1e-9 * absmax
    got32 = dnp.logits_batch(w, c, inp["tf_tokens"], inp["units"], dnp.N_FRAMES, dnp.TF_LEN, np.float32)
    assert got32.dtype == np.float32 and np.abs(got32 - ref).max() <= 4 * float(z[f"gap_{name}"]) * absmax
    rows = [1] if name != "B" else [0, 1, 2]      # (a cache-free decode is quadratic: one row of the wide configurations is enough)
    for b in rows:
        toks, lps, lg, margin = dnp.greedy_row(w, c, inp["units"][b, : dnp.N_FRAMES[b]], inp["prompts"][b], c["max_new"], inp["eos"], inp["suppress"],
                                               inp["begin_suppress"])
        n = int(z[f"gen_len_{name}"][b])
        assert toks == z[f"gen_tokens_{name}"][b, :n].tolist()
        assert np.abs(np.array(lps) - z[f"gen_lp_{name}"][b, : len(lps)]).max() <= 1e-9 * float(z[f"gen_absmax_{name}"])
        assert margin >= float(z[f"margin_{name}"]) * (1 - 1e-6) and float(z[f"margin_{name}"]) >= 1e-3      # (the recorded one is the smallest over the rows)
    assert float(z[f"hf_logits_{name}"]) < 1e-12      # the recipe's cross-check against transformers ran and agreed


def test_state_dict_keys_and_shapes():
    """Whisper(dims, decoder=True).state_dict() = the encoder's keys + the manifest's decoder keys (recorded from OpenAI's TextDecoder
    composed over the reference's blocks), for a small configuration and for large-v3; Whisper(dims) is what it was"""
    import torch
    from encoder.whisper.model import ModelDimensions, TextDecoder, Whisper
    from lds import arch
    enc_manifest = json.load(open(os.path.join(GOLDEN, "manifest_whisper.json")))
    c = dnp.CONFIGS["A"]
    dims = ModelDimensions(128, 1500, 128, 2, 4, c["n_vocab"], c["n_text_ctx"], c["n_state"], c["n_head"], c["n_layer"])
    plain, full = Whisper(dims), Whisper(dims, decoder=True)
    assert not hasattr(plain, "decoder")
    assert {k: list(v.shape) for k, v in plain.state_dict().items()} == enc_manifest["small"]
    dec = {k: list(v.shape) for k, v in full.state_dict().items() if k.startswith("decoder.")}
    assert dec == MANIFEST["shapes"]["A"] and list(dec) == list(MANIFEST["shapes"]["A"])
    assert {k: list(v.shape) for k, v in full.state_dict().items() if not k.startswith("decoder.")} == enc_manifest["small"]
    assert dict(arch.whisper_decoder_param_shapes(51866, 448, 1280, 32)) == {k: tuple(v) for k, v in MANIFEST["shapes"]["large_v3"].items()}
    with torch.device("meta"):
        big = Whisper(ModelDimensions(128, 1500, 1280, 20, 32, 51866, 448, 1280, 20, 32), decoder=True)
        assert Whisper(ModelDimensions(128, 1500, 1280, 20, 32, 51866, 448, 1280, 20, 32)).state_dict().keys() == enc_manifest["large_v3"].keys()
    sd = {k: list(v.shape) for k, v in big.state_dict().items()}
    assert sd == {**enc_manifest["large_v3"], **MANIFEST["shapes"]["large_v3"]}
    assert isinstance(big.decoder, TextDecoder) and big.is_multilingual and big.num_languages == 100
    # a full OpenAI model_state_dict loads both halves unchanged
    full.load_state_dict({k: torch.zeros(v) for k, v in {**enc_manifest["small"], **MANIFEST["shapes"]["A"]}.items()})


def test_python_refusals_need_no_device():
    import torch
    from encoder.whisper.model import ModelDimensions, Whisper
    c = dnp.CONFIGS["A"]
    dims = ModelDimensions(128, 1500, 128, 2, 1, c["n_vocab"], c["n_text_ctx"], c["n_state"], c["n_head"], c["n_layer"])
    xa = torch.zeros(1, 4, 128)
    with pytest.raises(RuntimeError, match="decoder=True"):
        Whisper(dims).logits(torch.zeros(1, 2, dtype=torch.int64), xa)
    m = Whisper(dims, decoder=True)
    for kw in (dict(temperature=0.2), dict(beam_size=5), dict(without_timestamps=False)):
        with pytest.raises(NotImplementedError):
            m.decode(xa, eot=1, prompt=[[0]], suppress_tokens=[], begin_suppress_tokens=[], **kw)
    with pytest.raises(RuntimeError, match="HIP device"):
        m.logits(torch.zeros(1, 2, dtype=torch.int64), xa)
    with pytest.raises(NotImplementedError, match="fp32"):
        m.decoder.cross(_FakeCuda(torch.float16))
    with pytest.raises(ValueError, match="multilingual"):
        m.special_tokens()


class _FakeCuda:
    """a stand-in with the two attributes TextDecoder.cross looks at before it touches the library"""
    is_cuda = True

    def __init__(self, dtype):
        self.dtype = dtype


def test_binding_mirrors_the_c_structs():
    """the struct definitions of include/lds.h against the ctypes mirrors: field names in order, and the size the C layout has"""
    from lds import native
    hdr = open(os.path.join(ROOT, "include", "lds.h")).read()
    m = re.search(r"typedef struct lds_whisper_decoder_cfg \{ int ([^;]+); \} lds_whisper_decoder_cfg;", hdr)
    assert [f.strip() for f in m.group(1).split(",")] == [f for f, _ in native.WhisperDecoderCfg._fields_]
    assert all(t is C.c_int for _, t in native.WhisperDecoderCfg._fields_) and C.sizeof(native.WhisperDecoderCfg) == 24
    body = re.search(r"typedef struct lds_whisper_decode_opts \{([^}]+)\} lds_whisper_decode_opts;", hdr).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [f.strip().lstrip("*").strip() for f in re.sub(r"^(const\s+)?\w+\s*\*?", "", decl, count=1).split(",")]
    assert fields == [f for f, _ in native.WhisperDecodeOpts._fields_]
    kinds = dict(native.WhisperDecodeOpts._fields_)
    assert kinds["suppress"] is C.c_void_p and kinds["begin_suppress"] is C.c_void_p and kinds["temperature"] is C.c_float
    assert C.sizeof(native.WhisperDecodeOpts) == 48 and native.WhisperDecodeOpts.suppress.offset == 16
    for name in ("lds_whisper_decoder_create", "lds_whisper_decoder_destroy", "lds_whisper_decoder_workspace_bytes", "lds_whisper_decoder_cross",
                 "lds_whisper_decoder_logits", "lds_whisper_decoder_generate"):
        assert name in native.EXPORTS and re.search(r"\b" + name + r"\(", hdr)
    assert "lds_test_whisper_head" in native.TEST_EXPORTS
    # argument counts of the table against the header's prototypes
    for name in ("lds_whisper_decoder_cross", "lds_whisper_decoder_logits", "lds_whisper_decoder_generate", "lds_whisper_decoder_workspace_bytes"):
        proto = re.search(r"\b" + name + r"\(([^;]*)\);", hdr).group(1)
        assert len(proto.split(",")) == len(native.SIGNATURES[name].split(":")[1]), name


def test_special_token_table():
    from lds import arch
    t = arch.whisper_special_tokens(51866)
    assert (t["eot"], t["sot"], t["translate"], t["transcribe"], t["startoflm"], t["startofprev"], t["nospeech"], t["notimestamps"], t["timestamp_begin"]) == \
        (50257, 50258, 50359, 50360, 50361, 50362, 50363, 50364, 50365)
    assert t["num_languages"] == 100 and t["languages"]["en"] == 50259 and t["languages"]["yue"] == 50358 and len(t["languages"]) == 100
    assert t["timestamp_begin"] + 1501 == 51866
    u = arch.whisper_special_tokens(51865)
    assert (u["num_languages"], u["translate"], u["transcribe"], u["notimestamps"], u["timestamp_begin"]) == (99, 50358, 50359, 50363, 50364)
    assert "yue" not in u["languages"] and u["timestamp_begin"] + 1501 == 51865 and u["languages"]["su"] == 50357
    assert len(set(arch.WHISPER_LANGUAGES)) == 100
    assert arch.whisper_special_tokens(51866, eot=7, notimestamps=9)["eot"] == 7
    with pytest.raises(TypeError):
        arch.whisper_special_tokens(51866, nonsense=1)
    with pytest.raises(ValueError):
        arch.whisper_special_tokens(51864)
    assert "UNVERIFIED" in arch.whisper_special_tokens.__doc__


def test_seeded_initialiser():
    from lds import arch
    a = arch.whisper_decoder_init_state(97, 16, 64, 1, seed=3)
    b = arch.whisper_decoder_init_state(97, 16, 64, 1, seed=3)
    assert list(a) == list(arch.whisper_decoder_param_shapes(97, 16, 64, 1)) and all(np.array_equal(a[k], b[k]) and a[k].dtype == np.float32 for k in a)
    assert not any(k.endswith("key.bias") for k in a)
    assert abs(np.abs(a["decoder.blocks.0.mlp.2.weight"]).max() - 3 / 16) < 1e-3      # 3 / sqrt(fan_in = 256)


def _tool():
    spec = importlib.util.spec_from_file_location("_transcribe_tool", os.path.join(ROOT, "tools", "transcribe.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_transcribe_parser(tmp_path, capsys):
    tool = _tool()
    ap = tool.build_parser()
    a = tool.check_args(ap, ap.parse_args([str(tmp_path), "--synthetic", "--layers", "2", "--language", "de", "--tokenizer", str(tmp_path)]))
    assert a.synthetic and a.layers == 2 and a.language == "de" and a.task == "transcribe" and a.tokenizer == str(tmp_path) and a.max_new_tokens == 224
    for argv, msg in (([str(tmp_path), "--synthetic", "--tokenizer", "openai/whisper-large-v3"], "hub name is refused"),
                      ([str(tmp_path)], "--checkpoint large-v3.pt or --synthetic"),
                      ([str(tmp_path), "--checkpoint", "x.pt", "--layers", "2"], "--layers belongs"),
                      ([str(tmp_path), "--synthetic", "--checkpoint", "x.pt"], "not allowed with"),
                      ([str(tmp_path), "--synthetic", "--task", "summarise"], "invalid choice"),
                      ([str(tmp_path), "--synthetic", "--batch", "65"], "1 .. 64")):
        with pytest.raises(SystemExit):
            tool.check_args(ap, ap.parse_args(argv))
        assert msg in capsys.readouterr().err
    src = open(os.path.join(ROOT, "tools", "transcribe.py")).read()
    assert src.count("from_pretrained(") == 1 and "local_files_only=True" in src


def test_host_side_selftest_under_sanitizers():
    """create (packing, the transposed head), the plans and every refusal of the four entries, run as csrc/whisper_dec_selftest.cpp with the host-only
    objects linked in (an ordinary executable that carries its sanitizer runtime: nothing is preloaded): a refusal that came after a launch would answer LDS_EHIP there"""
    csrc = os.path.join(PKG, "csrc")
    r = subprocess.run(["make", "-C", csrc, "-j8", "whisper_dec_selftest"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([os.path.join(csrc, "build_asan", "whisper_dec_selftest")], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "selftest passed" in p.stdout and "FAIL" not in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    assert "ERROR: " not in p.stderr and "runtime error:" not in p.stderr, p.stderr[-4000:]
