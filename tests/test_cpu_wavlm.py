"""The WavLM units encoder without a GPU: the numpy restatement against the fixtures recorded from transformers.WavLMModel in float64
(tests/golden/wavlm.npz), the library's bucket table against transformers' _relative_positions_bucket, the parameter table against the
recorded state-dict manifest (and against WavLMModel itself where transformers imports), the frame rule, the binding's mirror of
lds_wavlm_cfg, the argument checks that need no device, the Python refusals, the width table and the two tools' argument parsers."""
import ctypes
import importlib.util
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

import wavlm_numpy as wnp
from conftest import GOLDEN, ROOT

TOL64 = 1e-9      # x absmax: the float64 restatement against the float64 model, both stored in float64


@pytest.fixture(scope="module")
def z():
    return dict(np.load(os.path.join(GOLDEN, "wavlm.npz")))


@pytest.fixture(scope="module")
def manifest():
    return json.load(open(os.path.join(GOLDEN, "manifest_wavlm.json")))


_W = {}


def weights(flavour):
    from lds import arch
    if flavour not in _W:
        dims = wnp.dims_of(flavour, arch)
        _W[flavour] = (dims, arch.wavlm_init_state(dims, wnp.FIXTURE_SEED))
    return _W[flavour]


@pytest.mark.parametrize("clip", range(len(wnp.CLIPS)))
@pytest.mark.parametrize("flavour", wnp.FLAVOURS)
def test_numpy_restatement_reproduces_the_fixtures(flavour, clip, z):
    from lds import init_weights
    dims, w = weights(flavour)
    audio = wnp.make_clip(clip, init_weights.uniform)
    T = wnp.FRAMES[clip]
    assert len(audio) == wnp.CLIPS[clip][0] and wnp.frames_of(len(audio)) == T
    wave = wnp.normalize_wave(audio) if flavour == "large" else audio
    rows = z[f"{flavour}_rows_{clip}"]
    f64 = wnp.features(w, dims, wave, np.float64)
    got = {"feat": f64, "h1": wnp.encode(w, dims, wave, layer=1, dtype=np.float64, feats=f64),
           "last": wnp.encode(w, dims, wave, dtype=np.float64, feats=f64)}
    assert f64.shape == (T, 512) and got["last"].shape == got["h1"].shape == (T, dims["n_state"])
    for name, g in got.items():
        ref, am = z[f"{flavour}_{name}_{clip}"], float(z[f"{flavour}_absmax_{name}_{clip}"])
        assert ref.dtype == np.float64
        err = np.abs(g[rows] - ref).max() / am
        print(f"{flavour} clip {clip} {name}: {err:.2e} of absmax {am:.3f}")
        assert err < TOL64, (name, err)
    if T > 1:      # the restatement's own bias matters as much as the model's
        nb = wnp.encode(w, dims, wave, dtype=np.float64, feats=f64, zero_bias=True)
        moved = np.abs(nb - got["last"]).max() / np.abs(got["last"]).max()
        assert abs(moved - float(z[f"{flavour}_nobias_{clip}"])) < 1e-6 and moved >= 100 * 2e-5


def test_fixture_stages_live_at_a_scale_of_order_one_and_the_bias_matters(z):
    for fl in wnp.FLAVOURS:
        for i, T in enumerate(wnp.FRAMES):
            for name in ("feat", "h1", "last"):
                assert 0.1 < float(z[f"{fl}_absmax_{name}_{i}"]) < 100.0
                assert float(z[f"{fl}_gap_{name}_{i}"]) < 5e-6      # the model's own fp32-against-fp64 gap: the 2e-5 bound has room
            if T > 1:
                assert float(z[f"{fl}_nobias_{i}"]) >= 100 * 2e-5
            if T >= 75:
                lo, hi = z[f"{fl}_gate_{i}"]
                assert hi - lo >= 0.5
    assert os.path.getsize(os.path.join(GOLDEN, "wavlm.npz")) < (1 << 20)


def _torch_buckets(rel, num_buckets, max_distance):
    """transformers' WavLMAttention._relative_positions_bucket, or its text restated in torch where transformers is absent"""
    try:
        from transformers.models.wavlm.modeling_wavlm import WavLMAttention
        att = WavLMAttention.__new__(WavLMAttention)
        att.num_buckets, att.max_distance = num_buckets, max_distance
        return WavLMAttention._relative_positions_bucket(att, rel).numpy()
    except ImportError:
        import math
        nb = num_buckets // 2
        out = (rel > 0).to(torch.long) * nb
        a = torch.abs(rel)
        me = nb // 2
        big = torch.log(a.float() / me) / math.log(max_distance / me) * (nb - me)
        big = torch.min((me + big).to(torch.long), torch.full_like(a, nb - 1))
        return (out + torch.where(a < me, a, big)).numpy()


@pytest.mark.parametrize("num_buckets,max_distance", [(320, 800), (32, 80)])
def test_bucket_table_equals_transformers(num_buckets, max_distance):
    from lds import arch, native
    n = 1500
    want = _torch_buckets(torch.arange(-(n - 1), n), num_buckets, max_distance)
    got = np.zeros(2 * n - 1, dtype=np.int32)
    native.check(native.lib().lds_test_wavlm_buckets(num_buckets, max_distance, n, got.ctypes.data))
    assert np.array_equal(got, want)
    assert np.array_equal(arch.wavlm_buckets(num_buckets, max_distance, n), want)
    assert np.array_equal(wnp.buckets(np.arange(-(n - 1), n), num_buckets, max_distance), want)
    nb = num_buckets // 2
    assert want[0] == nb - 1 and want[-1] == num_buckets - 1 and want[n - 1] == 0      # both saturated buckets occur
    for bad in ((322, 800), (0, 800), (320, 80), (320, 0)):
        assert native.lib().lds_test_wavlm_buckets(bad[0], bad[1], n, got.ctypes.data) == -1


def test_frame_rule():
    from lds import arch, native
    from tools.tools import WavLMUnits
    for n in list(range(400, 3001)) + [480000]:
        assert WavLMUnits.frames_of(n) == native.WavLM.frames(n) == wnp.frames_of(n) == arch.hubert_level_frames(n, 0)[-1], n
    assert [WavLMUnits.frames_of(n) for n in (400, 16000, 480000)] == [1, 49, 1499]
    assert [WavLMUnits.frames_of(n) for n, _ in wnp.CLIPS] == list(wnp.FRAMES)
    assert WavLMUnits.min_samples == 400 and WavLMUnits.family == "WavLM" and WavLMUnits.NAMES == ("wavlmbase+", "wavlmlarge")


def test_shapes_and_keys_equal_the_manifest(manifest):
    from lds import arch
    for name in ("base+", "large"):
        shapes = {k: list(s) for k, s in arch.wavlm_param_shapes(arch.wavlm_dims(name)).items()}
        man = dict(manifest[name])
        assert man.pop("masked_spec_embed") == [arch.wavlm_dims(name)["n_state"]]      # not read
        assert shapes == man
    assert arch.wavlm_dims("base") == arch.wavlm_dims("base+")
    with pytest.raises(ValueError, match="wavlm_dims"):
        arch.wavlm_dims("huge")


def test_manifest_equals_transformers_state_dict(manifest):
    transformers = pytest.importorskip("transformers")
    with torch.device("meta"):
        m = transformers.WavLMModel(transformers.WavLMConfig())
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == manifest["base+"]


def test_binding_mirrors_the_header():
    from lds import native
    hdr = open(os.path.join(ROOT, "include", "lds.h")).read()
    m = re.search(r"typedef struct lds_wavlm_cfg \{ int ([^;]+); \} lds_wavlm_cfg;", hdr)
    fields = [f.strip() for f in m.group(1).split(",")]
    assert fields == [f for f, _ in native.WavlmCfg._fields_] == list(native.WavLM.FIELDS)
    assert fields == ["conv_dim", "n_state", "n_head", "n_layer", "n_ffn", "pos_kernel", "pos_groups", "num_buckets", "max_distance",
                      "stable_layer_norm", "n_ctx"]
    assert all(t is ctypes.c_int for _, t in native.WavlmCfg._fields_)
    sig = {"lds_wavlm_create": "i:pipppp", "lds_wavlm_destroy": "v:p", "lds_wavlm_workspace_bytes": "i:piqp", "lds_wavlm_features": "i:ppppipziqp",
           "lds_wavlm_encode": "i:ppppiipziqp"}
    for name, s in sig.items():
        assert name in native.EXPORTS and native.SIGNATURES[name] == s and len(re.findall(r"\b%s\(" % name, hdr)) == 1
        assert hasattr(native.lib(), name)
    thdr = open(os.path.join(ROOT, "include", "lds_test.h")).read()
    for name in ("lds_test_wavlm_attention", "lds_test_wavlm_buckets"):
        assert name in native.TEST_EXPORTS and len(re.findall(r"\b%s\(" % name, thdr)) == 1 and hasattr(native.lib(), name)
    for word in ("n_state = 64 n_head", "n_ctx <= 1500", "B <= 64", "num_buckets a multiple of 4"):
        assert word in hdr, word


def _tiny(stable=0):
    from lds import arch
    dims = dict(conv_dim=64, n_state=64, n_head=1, n_layer=1, n_ffn=64, pos_kernel=4, pos_groups=4, num_buckets=32, max_distance=80,
                stable_layer_norm=stable, n_ctx=1500)
    return dims, arch.wavlm_init_state(dims, 1)


def test_argument_checks_that_need_no_device():
    from lds import native
    L = native.lib()
    h, nb = ctypes.c_void_p(), ctypes.c_size_t()
    dims, _ = _tiny()
    cfg = native.WavlmCfg(*(dims[k] for k in native.WavLM.FIELDS))
    assert L.lds_wavlm_create(None, 0, None, None, None, ctypes.byref(h)) == -1
    for change, word in ((dict(num_buckets=30), "num_buckets"), (dict(max_distance=8), "max_distance"), (dict(stable_layer_norm=2), "stable_layer_norm"),
                         (dict(n_ctx=1501), "n_ctx"), (dict(n_head=2), "n_state / n_head"), (dict(n_layer=0), "n_layer")):
        bad = native.WavlmCfg(*(dict(dims, **change)[k] for k in native.WavLM.FIELDS))
        names, ptrs, numel = (ctypes.c_char_p * 1)(), (ctypes.c_void_p * 1)(), (ctypes.c_int64 * 1)()
        assert L.lds_wavlm_create(ctypes.byref(bad), 0, names, ptrs, numel, ctypes.byref(h)) == -1
        assert word in L.lds_last_error().decode(), (word, L.lds_last_error())
    assert cfg.n_ctx == 1500
    assert L.lds_wavlm_workspace_bytes(None, 1, 16000, ctypes.byref(nb)) == -1 and "null handle" in L.lds_last_error().decode()
    assert L.lds_wavlm_encode(None, None, None, None, 1, 0, None, 0, 1, 16000, None) == -1
    assert L.lds_wavlm_features(None, None, None, None, 0, None, 0, 1, 16000, None) == -1


@pytest.mark.parametrize("change,match", [
    (dict(conv_dim=96), "conv_dim"), (dict(n_state=1088, n_head=17), "n_state"), (dict(n_head=8), "64 \\* n_head"), (dict(n_ffn=100), "n_ffn"),
    (dict(pos_kernel=130), "pos_kernel"), (dict(pos_groups=8), "pos_groups"), (dict(n_layer=0), "n_layer"), (dict(n_ctx=1501), "n_ctx"),
    (dict(num_buckets=322), "num_buckets"), (dict(max_distance=80), "max_distance"), (dict(stable_layer_norm=2), "stable_layer_norm")])
def test_bad_dimensions_are_value_errors(change, match):
    from lds import arch, native
    with pytest.raises(ValueError, match=match):
        native.WavLM.check_dims(dict(arch.wavlm_dims("base+"), **change))


def test_units_encoder_construction_cases():
    from lds import arch
    from tools.tools import Units_Encoder, WavLMUnits, get_encdoer_out_channels
    for name in WavLMUnits.NAMES:
        with pytest.raises(NotImplementedError) as e:
            Units_Encoder(name)
        assert name in str(e.value) and "hub download" in str(e.value) and "checkpoint=PATH" in str(e.value)
    with pytest.raises(NotImplementedError, match="hub download"):
        WavLMUnits("wavlmlarge", device="cpu")
    with pytest.raises(ValueError, match="Unknown units encoder"):
        Units_Encoder("wavlmhuge", model=object())
    with pytest.raises(ValueError, match="units_layer= belongs to"):
        Units_Encoder("hubertsoft", model=object(), units_layer=3)
    assert get_encdoer_out_channels("wavlmbase+") == arch.get_encoder_out_channels("wavlmbase+") == 768
    assert get_encdoer_out_channels("wavlmlarge") == 1024
    assert [get_encdoer_out_channels(k) for k in ("whisper_large_v3", "contentvec768l12", "xlsr_53_56k", "hubertsoft")] == [1280, 768, 1024, 256]
    with pytest.raises(ValueError, match="Unknown encoder: w2v-bert"):      # (existing names and their errors stay as they are)
        get_encdoer_out_channels("w2v-bert")
    dims, state = _tiny()
    enc = Units_Encoder("wavlmbase+", device="cpu", model=WavLMUnits("wavlmbase+", device="cpu", dims=dims, state=state), units_layer=0)
    assert enc.model.hidden_dim == 64 and enc.min_samples == 400 and enc.model.n_ctx == 1500 and enc.model.frames_of(112240) == 350
    assert enc.model.units_layer == 0 and not enc.model.model.normalize
    big = WavLMUnits("wavlmlarge", device="cpu", dims=_tiny(1)[0], state=_tiny(1)[1])
    assert big.units_layer == 1 and big.model.normalize
    with pytest.raises(ValueError, match="units_layer 2 outside 0 .. 1"):
        WavLMUnits("wavlmbase+", device="cpu", dims=dims, state=state, units_layer=2)
    syn = WavLMUnits.synthetic("wavlmbase+", dims, seed=1, device="cpu")
    for k, v in syn.model.state_dict().items():
        assert np.array_equal(v.numpy(), state[k]), k
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc.encode(torch.zeros(16000), 16000)
    with pytest.raises(ValueError, match="lengths must be 2 integers in 400 .. 16000"):
        enc.model.encode_ragged(torch.zeros(2, 16000), [16000, 399])      # (the lengths are judged before the device)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc.encode_ragged(torch.zeros(2, 16000), [16000, 400])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc.model(torch.zeros(16000))


def test_cpu_tensors_masking_and_the_training_path_raise():
    from encoder.wavlm.model import WavLM
    from lds import native
    dims, state = _tiny()
    m = WavLM(dims, state=state)
    with pytest.raises(ValueError, match="exactly one of"):
        WavLM(dims)
    with pytest.raises(ValueError, match="exactly one of"):
        WavLM(dims, state=state, seed=1)
    assert np.array_equal(WavLM(dims, seed=1).state_dict()["encoder.layers.0.attention.gru_rel_pos_const"].numpy(),
                          state["encoder.layers.0.attention.gru_rel_pos_const"])
    for call in (m, m.encode, m.extract_features):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(torch.zeros(1, 16000))
    with pytest.raises(NotImplementedError, match="masking"):
        m(torch.zeros(1, 16000), mask_time_indices=torch.zeros(1, 49, dtype=torch.bool))
    with pytest.raises(NotImplementedError, match="attention_mask"):
        m(torch.zeros(1, 16000), attention_mask=torch.tensor([[1] * 15999 + [0]]))
    m.train()
    with pytest.raises(NotImplementedError, match="training path"):
        m(torch.zeros(1, 16000))
    h = native.WavLM.__new__(native.WavLM)
    h.dims, h.h, h.ws = dims, None, native.Workspace()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        h.encode(torch.zeros(1, 16000))
    with pytest.raises(ValueError, match="at least 400 samples"):
        h.encode(torch.zeros(1, 399))
    with pytest.raises(ValueError, match="more than n_ctx"):
        h.features(torch.zeros(1, 480400))
    with pytest.raises(ValueError, match="1 .. 64 clips"):
        h.encode(torch.zeros(65, 400))
    with pytest.raises(ValueError, match="layer 2 outside 0 .. 1"):
        h.encode(torch.zeros(1, 400), layer=2)


def test_checkpoints_load_and_a_missing_key_is_named(tmp_path):
    from tools.tools import Units_Encoder, WavLMUnits
    dims, state = _tiny(1)
    sd = {**{"wavlm." + k: torch.from_numpy(v) for k, v in state.items()}, "wavlm.masked_spec_embed": torch.zeros(64), "lm_head.weight": torch.zeros(4, 64)}
    p1, p2 = str(tmp_path / "a.pt"), str(tmp_path / "b.pt")
    torch.save(sd, p1)                      # a WavLMForCTC-style state dict: a prefix, the masking embedding and a head
    got = WavLMUnits("wavlmlarge", device="cpu", checkpoint=p1, dims=dims).model.state_dict()
    assert list(got) == list(state)
    for k, v in state.items():
        assert np.array_equal(got[k].numpy(), v), k
    bad = dict(sd)
    del bad["wavlm.encoder.layers.0.attention.rel_attn_embed.weight"]
    torch.save(bad, p2)
    with pytest.raises(KeyError, match="encoder.layers.0.attention.rel_attn_embed.weight"):
        WavLMUnits("wavlmlarge", device="cpu", checkpoint=p2, dims=dims)
    with pytest.raises(ValueError, match="feature_extractor.conv_layers.0.conv.weight"):      # the full-width network refuses it by shape
        Units_Encoder("wavlmlarge", device="cpu", checkpoint=p1)


def _tool(name):
    spec = importlib.util.spec_from_file_location("tool_" + name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tool_parsers_take_the_new_names(capsys):
    ex = _tool("extract_units").build_parser()
    a = ex.parse_args(["clips", "--encoder", "wavlmlarge", "--units_layer", "6", "--synthetic"])
    assert (a.encoder, a.units_layer, a.synthetic) == ("wavlmlarge", 6, True)
    assert ex.parse_args(["clips", "--encoder", "wavlmbase+"]).units_layer is None
    assert ex.parse_args(["clips"]).encoder == "whisper_large_v3"
    bu = _tool("bench_units")
    assert bu.parse_args([]).encoder == "whisper_large_v3"
    for name in ("wavlmbase+", "wavlmlarge", "contentvec768l12"):
        assert bu.parse_args(["--encoder", name, "--layers", "2"]).encoder == name
    with pytest.raises(SystemExit):
        bu.parse_args(["--encoder", "wavlmhuge"])
    sys.path.insert(0, ROOT)
    try:
        import infer_svc
    finally:
        sys.path.remove(ROOT)
    assert infer_svc.parse_args(["--encoder", "wavlmbase+", "--synthetic"]).encoder == "wavlmbase+"
    capsys.readouterr()
