"""The w2v-BERT 2.0 units encoder without a GPU: the numpy restatement (front end and model) against the fixtures recorded from
transformers' SeamlessM4TFeatureExtractor and Wav2Vec2BertModel (tests/golden/w2vbert.npz), the frame rule against the extractor on a
sweep of lengths, the key table against the recorded state-dict manifest, the binding's mirror of lds_w2vbert_cfg, the Units_Encoder
construction cases, a checkpoint round trip, and the refusal of CPU tensors."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import w2vbert_numpy as wnp
from conftest import GOLDEN, ROOT

TOL64 = 1e-6      # x absmax: the float64 restatement against the recorded outputs


@pytest.fixture(scope="module")
def weights():
    from lds import arch
    dims = dict(arch.W2V_BERT_DIMS, n_layer=wnp.FIXTURE_LAYERS)
    return dims, arch.w2vbert_init_state(dims, wnp.FIXTURE_SEED)


@pytest.fixture(scope="module")
def z():
    return dict(np.load(os.path.join(GOLDEN, "w2vbert.npz")))


@pytest.fixture(scope="module")
def manifest():
    return json.load(open(os.path.join(GOLDEN, "manifest_w2vbert.json")))


@pytest.mark.parametrize("clip", [0, 1, 2, 3, 4])
def test_numpy_restatement_reproduces_the_fixtures(clip, weights, z):
    """the front end in the extractor's own float32 arithmetic and the model in float64 on those features: within 1e-6 absmax of the recorded
    input_features and last_hidden_state; the float64 front end within the extractor's recorded float32 gap"""
    from lds import init_weights
    dims, w = weights
    audio = wnp.make_clip(clip, init_weights.uniform)
    n, valid, R = wnp.frames_of(len(audio))
    assert len(audio) == wnp.CLIPS[clip][0] and (n, R) == (wnp.FRAMES[clip], wnp.ROWS[clip]) and valid == n // 2
    rows = z[f"rows_{clip}"]
    f32, f64 = wnp.fbank(audio, dtype=np.float32), wnp.fbank(audio)
    assert f32.shape == f64.shape == (R, 160) and f32.dtype == np.float32
    am = float(z[f"absmax_feats_{clip}"])
    ref = z[f"feats_{clip}"].astype(np.float64)
    err32, err64 = np.abs(f32[rows] - ref).max() / am, np.abs(f64[rows] - ref).max() / am
    print(f"clip {clip} feats: float32 arithmetic {err32:.2e}, float64 {err64:.2e} of absmax {am:.3f} (recorded gap {float(z[f'gap_feats_{clip}']):.2e})")
    assert err32 < TOL64, err32
    assert err64 <= float(z[f"gap_feats_{clip}"]) * (1 + 1e-9) + 1e-12
    if n % 2:
        assert not f32[-1, 80:].any() and not f64[-1, 80:].any()      # the masked row's padding
    e64 = wnp.encode(w, dims, f32, n, np.float64)
    assert e64.shape == (R, 1024)
    am = float(z[f"absmax_enc_{clip}"])
    err = np.abs(e64[rows] - z[f"enc_{clip}"].astype(np.float64)).max() / am
    print(f"clip {clip} enc: {err:.2e} of absmax {am:.3f}")
    assert err < TOL64, err


def test_fixture_stages_live_at_a_scale_of_order_one(z):
    for i in range(5):
        for name in ("feats", "enc"):
            assert 0.1 < float(z[f"absmax_{name}_{i}"]) < 100.0
        assert float(z[f"gap_enc_{i}"]) < 5e-6 and float(z[f"gap_feats_{i}"]) < 1e-5


def test_frame_rule_against_the_extractor():
    """(n, valid, rows) of lds.arch.w2vbert_frames against SeamlessM4TFeatureExtractor's own shapes and mask on a sweep of lengths"""
    transformers = pytest.importorskip("transformers")
    from lds import arch
    from tools.tools import Wav2Vec2Bert
    fe = transformers.SeamlessM4TFeatureExtractor()
    rng = np.random.default_rng(0)
    for L in [560, 561, 719, 720, 721, 879, 880, 1040, 1199, 1200, 1999, 4000, 16000]:
        x = rng.standard_normal(L).astype(np.float32)
        o = fe(x, sampling_rate=16000, return_tensors="np")
        n, valid, rows = arch.w2vbert_frames(L)
        assert o["input_features"].shape == (1, rows, 160) and int(o["attention_mask"].sum()) == valid, L
        assert wnp.frames_of(L) == (n, valid, rows) and Wav2Vec2Bert.frames_of(L) == rows
    assert [arch.w2vbert_frames(L) for L in (560, 720, 24240, 24400, 64240, 480000)] == [(2, 1, 1), (3, 1, 2), (150, 75, 75), (151, 75, 76), (400, 200, 200),
                                                                                        (2998, 1499, 1499)]
    assert arch.W2VBERT_MIN_SAMPLES == Wav2Vec2Bert.min_samples == 560 and Wav2Vec2Bert.family == "w2v-BERT"


def test_shapes_and_keys_equal_the_manifest(manifest):
    from lds import arch
    shapes = arch.w2vbert_param_shapes()
    hf = manifest["transformers"]
    assert set(shapes) | {"masked_spec_embed"} == set(hf)
    for k, s in shapes.items():
        assert list(s) == hf[k], k
    assert arch.W2V_BERT_DIMS["n_state"] == 1024 and arch.W2V_BERT_DIMS["n_layer"] == 24


def test_binding_mirrors_the_header():
    from lds import native
    hdr = open(os.path.join(ROOT, "include", "lds.h")).read()
    m = re.search(r"typedef struct lds_w2vbert_cfg \{ int ([^;]+); float eps; \} lds_w2vbert_cfg;", hdr)
    fields = [f.strip() for f in m.group(1).split(",")]
    assert fields + ["eps"] == [f for f, _ in native.W2vBertCfg._fields_] == list(native.Wav2Vec2Bert.FIELDS) + ["eps"]
    assert all(t is ctypes.c_int for _, t in native.W2vBertCfg._fields_[:-1]) and native.W2vBertCfg._fields_[-1][1] is ctypes.c_float
    for name in ("lds_w2vbert_create", "lds_w2vbert_destroy", "lds_w2vbert_workspace_bytes", "lds_w2vbert_fbank", "lds_w2vbert_encode_features",
                 "lds_w2vbert_encode"):
        assert name in native.EXPORTS and len(re.findall(r"\b%s\(" % name, hdr)) == 1
        assert hasattr(native.lib(), name)
    thdr = open(os.path.join(ROOT, "include", "lds_test.h")).read()
    for name in ("lds_test_w2vbert_fbank", "lds_test_w2vbert_attention", "lds_test_w2vbert_dwconv"):
        assert name in native.TEST_EXPORTS and len(re.findall(r"\b%s\(" % name, thdr)) == 1 and hasattr(native.lib(), name)


@pytest.mark.parametrize("change,match", [
    (dict(n_mels=81), "n_mels"), (dict(n_state=1088, n_head=17), "n_state"), (dict(n_head=8), "n_head"), (dict(n_ffn=100), "n_ffn"),
    (dict(left_max=72), "left_max"), (dict(dw_kernel=30), "dw_kernel"), (dict(dw_kernel=33), "dw_kernel"), (dict(n_layer=0), "n_layer"),
    (dict(n_ctx=1501), "n_ctx"), (dict(eps=0.0), "eps")])
def test_bad_dimensions_are_value_errors(change, match):
    from lds import arch, native
    with pytest.raises(ValueError, match=match):
        native.Wav2Vec2Bert.check_dims(dict(arch.W2V_BERT_DIMS, **change))


def _tiny():
    from lds import arch
    dims = dict(arch.W2V_BERT_DIMS, n_state=64, n_head=1, n_ffn=64, n_layer=1)
    return dims, arch.w2vbert_init_state(dims, 1)


def test_units_encoder_construction_cases():
    from tools.tools import Units_Encoder, Wav2Vec2Bert
    with pytest.raises(NotImplementedError) as e:
        Units_Encoder("w2v-bert")
    assert "w2v-bert" in str(e.value) and "transformers" in str(e.value)
    with pytest.raises(NotImplementedError, match="transformers"):
        Units_Encoder("w2v-bert", device="cpu", resample=True)
    with pytest.raises(NotImplementedError, match="w2v-bert"):
        Wav2Vec2Bert(device="cpu")
    dims, state = _tiny()
    enc = Units_Encoder("w2v-bert", device="cpu", model=Wav2Vec2Bert(device="cpu", dims=dims, state=state))
    assert enc.model.hidden_dim == 64 and enc.min_samples == 560 and enc.model.n_ctx == 1500 and enc.model.frames_of(24400) == 76
    syn = Wav2Vec2Bert.synthetic(dims, seed=1, device="cpu")
    for k, v in syn.model.state_dict().items():
        assert np.array_equal(v.numpy(), state[k]), k
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc.encode(torch.zeros(16000), 16000)
    with pytest.raises(ValueError, match="lengths must be 2 integers in 560 .. 16000"):
        enc.model.encode_ragged(torch.zeros(2, 16000), [16000, 559])      # (the lengths are judged before the device)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc.encode_ragged(torch.zeros(2, 16000), [16000, 560])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc.model(torch.zeros(16000))


def test_argument_checks_raise_before_any_handle_is_used():
    from encoder.wav2vec2_bert.model import Wav2Vec2BertModel
    from lds import native
    dims, state = _tiny()
    m = Wav2Vec2BertModel(dims)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 10, 160))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.encode_audio(torch.zeros(1, 16000))
    h = native.Wav2Vec2Bert.__new__(native.Wav2Vec2Bert)
    h.dims, h.h, h.ws = native.Wav2Vec2Bert.check_dims(dims), None, native.Workspace()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        h.encode(torch.zeros(1, 16000))
    with pytest.raises(ValueError, match="at least 560 samples"):
        h.encode(torch.zeros(1, 559))
    with pytest.raises(ValueError, match="more than n_ctx"):
        h.fbank(torch.zeros(1, 480400))
    with pytest.raises(ValueError, match="1 .. 64 clips"):
        h.encode(torch.zeros(65, 560))
    with pytest.raises(ValueError, match=r"features must be \[B, R, 160\]"):
        h.encode_features(torch.zeros(1, 10, 80))
    with pytest.raises(ValueError, match="lengths must be 1 integers in 2 .. 20"):
        h.encode_features(torch.zeros(1, 10, 160), [21])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        h.encode_features(torch.zeros(1, 10, 160), [19])


def test_checkpoint_round_trip_and_a_missing_key_is_named(tmp_path):
    from tools.tools import Units_Encoder, Wav2Vec2Bert
    dims, state = _tiny()
    sd = {k: torch.from_numpy(v) for k, v in state.items()}
    sd["masked_spec_embed"] = torch.zeros(64)      # dropped on load
    paths = [str(tmp_path / "ck0.pt"), str(tmp_path / "ck1.pt")]
    torch.save(sd, paths[0])
    torch.save({"state_dict": {"wav2vec2_bert." + k: v for k, v in sd.items()}}, paths[1])
    try:
        from safetensors.torch import save_file
        paths.append(str(tmp_path / "ck2.safetensors"))
        save_file({k: v.contiguous() for k, v in sd.items()}, paths[-1])
    except ImportError:
        pass
    for path in paths:
        m = Wav2Vec2Bert(device="cpu", checkpoint=path, dims=dims)
        got = m.model.state_dict()
        assert list(got) == list(state)
        for k, v in state.items():
            assert np.array_equal(got[k].numpy(), v), k
    bad = dict(sd)
    del bad["encoder.layers.0.conv_module.depthwise_conv.weight"]
    p3 = str(tmp_path / "ck3.pt")
    torch.save(bad, p3)
    with pytest.raises(KeyError, match="encoder.layers.0.conv_module.depthwise_conv.weight"):
        Wav2Vec2Bert(device="cpu", checkpoint=p3, dims=dims)
    # Units_Encoder(checkpoint=) builds the full-width network: a checkpoint of other widths is refused by shape, naming the tensor
    with pytest.raises(ValueError, match="feature_projection.projection.weight"):
        Units_Encoder("w2v-bert", device="cpu", checkpoint=paths[0])
