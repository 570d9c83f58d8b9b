"""The XLSR-53 (wav2vec 2.0, layer-norm flavour) units encoder without a GPU: the numpy restatement against the fixtures recorded from
transformers.Wav2Vec2Model in float64 (tests/golden/xlsr.npz), the key tables against the recorded state-dict manifest, the frame rule,
the binding's mirror of lds_w2v_cfg, the Units_Encoder construction cases, checkpoint loading in both namings, and the refusal of CPU
tensors."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import w2v_numpy as wnp
from conftest import GOLDEN, ROOT

TOL64 = 1e-6      # x absmax: the float64 restatement against the float64 model (DESIGN section 22's figure for the HuBERT restatement)


@pytest.fixture(scope="module")
def weights():
    from lds import arch
    dims = dict(arch.XLSR_53_DIMS, n_layer=wnp.FIXTURE_LAYERS)
    return dims, arch.w2v_init_state(dims, wnp.FIXTURE_SEED)


@pytest.fixture(scope="module")
def z():
    return dict(np.load(os.path.join(GOLDEN, "xlsr.npz")))


@pytest.fixture(scope="module")
def manifest():
    return json.load(open(os.path.join(GOLDEN, "manifest_xlsr.json")))


@pytest.mark.parametrize("clip", [0, 1, 2, 3, 4])
def test_numpy_restatement_reproduces_the_fixtures(clip, weights, z):
    from lds import init_weights
    dims, w = weights
    audio = wnp.make_clip(clip, init_weights.uniform)
    assert len(audio) == wnp.CLIPS[clip][0] and wnp.frames_of(len(audio)) == wnp.FRAMES[clip]
    rows = z[f"rows_{clip}"]
    f64 = wnp.features(w, audio, np.float64)
    e64 = wnp.encode(w, dims, audio, np.float64, feats=f64)
    assert f64.shape == (wnp.FRAMES[clip], 512) and e64.shape == (wnp.FRAMES[clip], 1024)
    for name, got in (("feat", f64), ("enc", e64)):
        ref, am = z[f"{name}_{clip}"].astype(np.float64), float(z[f"absmax_{name}_{clip}"])
        err = np.abs(got[rows] - ref).max() / am
        print(f"clip {clip} {name}: {err:.2e} of absmax {am:.3f}")
        assert err < TOL64, (name, err)


def test_fixture_stages_live_at_a_scale_of_order_one(z):
    for i in range(5):
        for name in ("feat", "enc"):
            assert 0.1 < float(z[f"absmax_{name}_{i}"]) < 100.0
            assert float(z[f"gap_{name}_{i}"]) < 5e-6      # the model's own fp32-against-fp64 gap: the 2e-5 bound has room


def test_frame_rule():
    from lds import arch, native
    from tools.tools import Audio2xlsr_53_56k
    for n in list(range(400, 3001)) + [480000]:
        lv = arch.hubert_level_frames(n, 0)
        assert Audio2xlsr_53_56k.frames_of(n) == native.Wav2Vec2.frames(n) == wnp.frames_of(n) == lv[-1], n
    assert [Audio2xlsr_53_56k.frames_of(n) for n in (400, 1279, 16000, 41277, 61760, 112077, 480000)] == [1, 3, 49, 128, 192, 349, 1499]
    assert Audio2xlsr_53_56k.min_samples == 400 and Audio2xlsr_53_56k.family == "wav2vec 2.0"


def test_shapes_and_keys_equal_the_manifest_and_the_tables_round_trip(manifest):
    from lds import arch
    shapes = arch.w2v_param_shapes()
    assert {k: list(s) for k, s in shapes.items()} == manifest["fairseq"]
    hf = manifest["transformers"]
    fwd = {k: arch.w2v_key_to_transformers(k) for k in shapes}
    back = arch.w2v_keys_from_transformers()
    assert len(set(fwd.values())) == len(fwd)                                   # one to one
    assert set(fwd.values()) | {"masked_spec_embed"} == set(hf)                 # onto the model's state dict
    assert set(back) == set(hf) and back["masked_spec_embed"] == "mask_emb"
    for k, t in fwd.items():
        assert back[t] == k and list(shapes[k]) == hf[t], (k, t)
    assert arch.w2v_key_to_transformers("mask_emb") == "masked_spec_embed"
    assert arch.get_encoder_out_channels("xlsr_53_56k") == arch.XLSR_53_DIMS["n_state"] == 1024


def test_binding_mirrors_the_header():
    from lds import native
    hdr = open(os.path.join(ROOT, "include", "lds.h")).read()
    m = re.search(r"typedef struct lds_w2v_cfg \{ int ([^;]+); \} lds_w2v_cfg;", hdr)
    fields = [f.strip() for f in m.group(1).split(",")]
    assert fields == [f for f, _ in native.W2vCfg._fields_] == list(native.Wav2Vec2.FIELDS)
    assert all(t is ctypes.c_int for _, t in native.W2vCfg._fields_)
    for name in ("lds_w2v_create", "lds_w2v_destroy", "lds_w2v_workspace_bytes", "lds_w2v_features", "lds_w2v_encode"):
        assert name in native.EXPORTS and len(re.findall(r"\b%s\(" % name, hdr)) == 1
        assert hasattr(native.lib(), name)
    thdr = open(os.path.join(ROOT, "include", "lds_test.h")).read()
    for name in ("lds_test_w2v_conv0", "lds_test_w2v_ln_act"):
        assert name in native.TEST_EXPORTS and len(re.findall(r"\b%s\(" % name, thdr)) == 1 and hasattr(native.lib(), name)


@pytest.mark.parametrize("change,match", [
    (dict(conv_dim=96), "conv_dim"), (dict(n_state=1088, n_head=17), "n_state"), (dict(n_head=8), "64 \\* n_head"), (dict(n_ffn=100), "n_ffn"),
    (dict(pos_kernel=130), "pos_kernel"), (dict(pos_groups=8), "pos_groups"), (dict(n_layer=0), "n_layer"), (dict(n_ctx=1501), "n_ctx")])
def test_bad_dimensions_are_value_errors(change, match):
    from lds import arch, native
    with pytest.raises(ValueError, match=match):
        native.Wav2Vec2.check_dims(dict(arch.XLSR_53_DIMS, **change))


class _CfgLikeFairseqs:
    """stands for the configuration objects a fairseq checkpoint pickles next to its weights"""


def _tiny():
    from lds import arch
    dims = dict(conv_dim=64, n_state=64, n_head=1, n_layer=1, n_ffn=64, pos_kernel=4, pos_groups=4, n_ctx=1500)
    return dims, arch.w2v_init_state(dims, 1)


def test_units_encoder_construction_cases():
    from tools.tools import Audio2xlsr_53_56k, Units_Encoder
    with pytest.raises(NotImplementedError) as e:
        Units_Encoder("xlsr_53_56k")
    assert "xlsr_53_56k" in str(e.value) and "fairseq" in str(e.value)
    with pytest.raises(NotImplementedError, match="fairseq"):
        Units_Encoder("xlsr_53_56k", device="cpu", resample=True)
    dims, state = _tiny()
    enc = Units_Encoder("xlsr_53_56k", device="cpu", model=Audio2xlsr_53_56k(device="cpu", dims=dims, state=state))
    assert enc.model.hidden_dim == 64 and enc.min_samples == 400 and enc.model.n_ctx == 1500 and enc.model.frames_of(112077) == 349
    syn = Audio2xlsr_53_56k.synthetic(dims, seed=1, device="cpu")
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


def test_cpu_tensors_and_the_training_path_raise():
    from encoder.wav2vec2.model import Wav2Vec2
    dims, state = _tiny()
    m = Wav2Vec2(dims)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.extract_features(torch.zeros(1, 16000))
    with pytest.raises(NotImplementedError, match="training path"):
        m(torch.zeros(1, 16000))
    from lds import native
    h = native.Wav2Vec2.__new__(native.Wav2Vec2)
    h.dims, h.h, h.ws = dims, None, native.Workspace()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        h.encode(torch.zeros(1, 16000))
    with pytest.raises(ValueError, match="at least 400 samples"):
        h.encode(torch.zeros(1, 399))
    with pytest.raises(ValueError, match="more than n_ctx"):
        h.features(torch.zeros(1, 480400))
    with pytest.raises(ValueError, match="at most 64 clips"):
        h.encode(torch.zeros(65, 400), [400] * 65)


def test_checkpoints_in_both_namings_load_and_a_missing_key_is_named(tmp_path):
    from lds import arch
    from tools.tools import Audio2xlsr_53_56k, Units_Encoder
    dims, state = _tiny()
    extra = {"mask_emb": torch.zeros(64), "quantizer.vars": torch.zeros(1, 8, 4), "quantizer.weight_proj.weight": torch.zeros(8, 64),
             "project_q.weight": torch.zeros(4, 4), "final_proj.bias": torch.zeros(4)}
    fair = {**{k: torch.from_numpy(v) for k, v in state.items()}, **extra}
    p1, p2, p3, p4 = (str(tmp_path / f"ck{i}.pt") for i in range(4))
    torch.save({"model": fair, "args": None}, p1)                       # fairseq's layout, re-saved without its classes
    hf = {arch.w2v_key_to_transformers(k): v for k, v in fair.items() if not k.startswith(("quantizer", "project_q", "final_proj"))}
    torch.save(hf, p2)                                                   # a bare state dict in transformers naming
    for path in (p1, p2):
        m = Audio2xlsr_53_56k(device="cpu", checkpoint=path, dims=dims)
        got = m.model.state_dict()
        assert list(got) == list(state)
        for k, v in state.items():
            assert np.array_equal(got[k].numpy(), v), k
    bad = dict(fair)
    del bad["encoder.layers.0.fc1.bias"]
    torch.save(bad, p3)
    with pytest.raises(KeyError, match="encoder.layers.0.fc1.bias"):
        Audio2xlsr_53_56k(device="cpu", checkpoint=p3, dims=dims)
    # Units_Encoder(checkpoint=) builds the full-width network: a checkpoint of other widths is refused by shape, naming the tensor
    with pytest.raises(ValueError, match="feature_extractor.conv_layers.0.0.weight"):
        Units_Encoder("xlsr_53_56k", device="cpu", checkpoint=p1)
    torch.save({"cfg": _CfgLikeFairseqs(), "model": fair}, p4)      # a pickle that needs a class the safe loader does not know
    with pytest.raises(RuntimeError, match="re-save the weights alone"):
        Audio2xlsr_53_56k(device="cpu", checkpoint=p4, dims=dims)


def test_plan_long_audio_works_with_this_encoder():
    from tools.infer_tools import DiffusionSVC
    from tools.tools import Audio2xlsr_53_56k, Units_Encoder
    dims, state = _tiny()
    ranges = [(0, 0, 30000), (170, 31000, 31500), (180, 33000, 63000), (400, 70000, 78000)]
    svc = DiffusionSVC(device="cpu")
    svc.args = {"data": {"block_size": 512, "sampling_rate": 44100}}
    svc.units_encoder = Units_Encoder("xlsr_53_56k", device="cpu", resample=True, model=Audio2xlsr_53_56k(device="cpu", dims=dims, state=state))
    plan = svc._plan_long_audio(44100, ranges, batch_size=3)
    assert plan["hop_size"] == 512.0 and plan["n_frames"] == [59, 1, 59, 16] and plan["chunks"] == [[1, 3, 0], [2]]
    # 1500 frames need 400 + 320 * 1499 = 480,080 samples; one frame more is over the window
    svc._plan_long_audio(16000, [(0, 0, 480399)], batch_size=1)
    with pytest.raises(ValueError, match=r"segment 0 .*exceeds the units encoder's window of 1500 frames \(30 s for wav2vec 2.0\)"):
        svc._plan_long_audio(16000, [(0, 0, 480400)], batch_size=1)
