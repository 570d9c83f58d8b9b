"""The x-vector speaker head without a GPU: the float64 restatement (tests/xvector_numpy.py) against the fixture recorded from
transformers' WavLMForXVector, every refusal of the C ABI and of the Python classes (argument checks run before any device call), the
key-stripping helper and the checkpoint loader."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import xvector_numpy as XN

torch = pytest.importorskip("torch")


def head_state(D=768, n_layer=None, **kw):
    from lds import arch
    return arch.xvector_init_state(D, XN.HEAD_SEED, n_layer, **kw)


def test_restatement_equals_the_fixture(golden):
    """the head restated in numpy, on the stored float64 input of the 16-frame clip (T_out = 2), against WavLMForXVector's own embeddings and
    logits: 1e-12 x absmax.  (The generator asserts the same for all three models on all four clips.)"""
    fx = golden("xvector.npz")
    hidden = fx["base_sum.hidden0"]
    assert hidden.dtype == np.float64 and hidden.shape == (XN.FRAMES[0], 768)
    emb, logits = XN.head(head_state(768, 2), hidden)
    am = fx["base_sum.absmax"]
    assert np.abs(emb - fx["base_sum.embeddings"][0]).max() <= 1e-12 * am[0]
    assert np.abs(logits - fx["base_sum.logits"][0]).max() <= 1e-12 * am[1]


def test_fixture_is_consistent(golden):
    fx = golden("xvector.npz")
    for m in XN.MODELS:
        emb = fx[f"{m}.embeddings"]
        assert emb.shape == (4, 512) and fx[f"{m}.logits"].shape == (4, XN.N_LABELS)
        assert np.abs(XN.cosine(emb, emb) - fx[f"{m}.cosine"]).max() < 1e-12
        assert np.all(fx[f"{m}.gap"] < 2e-5) and np.all(fx[f"{m}.gap"] > 0)      # the model's own fp32 sits well inside the GPU suite's bound
        off = fx[f"{m}.cosine"][~np.eye(4, dtype=bool)]
        assert off.max() < 1 - 1e-5      # the clips' embeddings differ by far more than the bound


def test_restatement_pieces():
    rng = np.random.default_rng(0)
    x, W, b = rng.standard_normal((20, 6)), rng.standard_normal((5, 18)), rng.standard_normal(5)
    y = XN.tdnn(x, W, b, 3, 2)
    ref = torch.relu(torch.nn.functional.conv1d(torch.from_numpy(x.T)[None], torch.from_numpy(W).view(5, 3, 6).transpose(1, 2), torch.from_numpy(b), dilation=2))[0].T
    assert y.shape == (16, 5) and np.abs(y - ref.numpy()).max() < 1e-12
    p = XN.pool(y)
    assert np.abs(p[5:] - torch.from_numpy(y).std(dim=0).numpy()).max() < 1e-12
    with pytest.raises(ValueError, match="2 frames"):
        XN.pool(y[:1])
    a = rng.standard_normal((3, 7))
    assert np.abs(XN.cosine(a, a[:2]) - torch.nn.functional.cosine_similarity(torch.from_numpy(a)[:, None], torch.from_numpy(a[:2])[None], dim=-1).numpy()).max() < 1e-12
    assert XN.cosine(np.zeros((1, 4)), np.ones((1, 4)))[0, 0] == 0.0


# ---- refusals, device-free ----
@pytest.fixture(scope="module")
def lib():
    from lds import native
    return native.lib()


def _refused(lib, rc, code, *words):
    msg = lib.lds_last_error().decode()
    assert rc == code, (rc, msg)
    for w in words:
        assert w in msg, msg


def _cfg(d_in=64, dims=(64, 64), kernels=(3, 1), dilations=(2, 1), xdim=32):
    from lds import native
    arr = lambda v: (C.c_int * 8)(*(list(v) + [0] * 8)[:8])
    return native.XVectorCfg(d_in, len(dims), arr(dims), arr(kernels), arr(dilations), xdim)


def _tiny_state(d_in=64, dims=(64, 64), kernels=(3, 1), xdim=32, labels=8):
    from lds import arch
    return arch.xvector_init_state(d_in, 0, None, labels, dict(tdnn_dim=dims, tdnn_kernel=kernels, tdnn_dilation=(2, 1), xvector_output_dim=xdim))


def _create(lib, cfg, state):
    from lds import native
    n, names, ptrs, numel, keep = native._host_tensor_table(state)
    h = C.c_void_p()
    return lib.lds_xvector_create(C.byref(cfg), n, names, ptrs, numel, C.byref(h)), h


def test_c_abi_refusals(lib):
    """every check comes before anything is enqueued (the data pointers are host memory: nothing may touch them).  lds_xvector_create only
    uploads the weights, so the cases that need a handle run where a HIP device exists (tests/test_gpu_xvector.py)."""
    one = (C.c_int32 * 65)(*([20] * 65))
    buf = C.create_string_buffer(1 << 16)
    p = C.cast(buf, C.c_void_p)
    nb = C.c_size_t()
    st = _tiny_state()
    # bad cfg
    _refused(lib, _create(lib, _cfg(dims=()), st)[0], -1, "n_tdnn 0")
    _refused(lib, _create(lib, _cfg(d_in=48), st)[0], -1, "Cin 48", "K-step 32")
    _refused(lib, _create(lib, _cfg(dims=(80, 64)), st)[0], -1, "Cin 80", "K-step 32")
    _refused(lib, _create(lib, _cfg(dims=(64, 66)), st)[0], -1, "Cout 66")
    _refused(lib, _create(lib, _cfg(kernels=(9, 1)), st)[0], -1, "kernel size 9")
    _refused(lib, _create(lib, _cfg(dilations=(0, 1)), st)[0], -1, "dilation 0")
    _refused(lib, _create(lib, _cfg(xdim=30), st)[0], -1, "xvector_dim 30")
    _refused(lib, lib.lds_xvector_create(None, 0, None, None, None, None), -1, "null")
    # a missing tensor is named; so is one of the wrong size
    short = {k: v for k, v in st.items() if k != "tdnn.1.kernel.bias"}
    rc, _ = _create(lib, _cfg(), short)
    if rc != -3 and rc != -2:      # (without a HIP device the first upload fails before the table is complete)
        _refused(lib, rc, -4, "tdnn.1.kernel.bias (absent)")
    # the one-layer entries: Cin not a multiple of the K-step, sizes, lengths, NULL
    tdnn = lambda B, T, Cin, Cout, ks, d, nf=one, X=p: lib.lds_test_xvector_tdnn(X, B, T, nf, p, p, Cin, Cout, ks, d, 1, p, None)
    _refused(lib, tdnn(1, 20, 48, 64, 1, 1), -1, "Cin 48", "K-step 32", "two taps")
    _refused(lib, tdnn(1, 20, 64, 62, 1, 1), -1, "Cout 62")
    _refused(lib, tdnn(65, 20, 64, 64, 1, 1), -1, "B 65")
    _refused(lib, tdnn(1, 0, 64, 64, 1, 1), -1, "T 0")
    _refused(lib, tdnn(1, 40000, 64, 64, 1, 1), -1, "T 40000")
    _refused(lib, tdnn(2, 20, 64, 64, 1, 1, (C.c_int32 * 2)(3, 21)), -1, "n_frames[1] = 21")
    _refused(lib, tdnn(1, 20, 64, 64, 1, 1, None), -1, "null n_frames")
    _refused(lib, tdnn(1, 20, 64, 64, 1, 1, one, None), -1, "null pointer")
    assert lib.lds_test_xvector_pool_workspace_bytes(2, 300, 1500, C.byref(nb)) == 0 and nb.value >= 2 * 6 * 1500 * 8
    need = nb.value
    pool = lambda nf, ws: lib.lds_test_xvector_pool(p, 2, 300, nf, p, p, 64, 1500, 3, 2, p, None, p, ws, None)
    _refused(lib, pool((C.c_int32 * 2)(300, 5), need), -1, "n_frames[1] = 5", "1 pooled frames")      # T_out < 2
    _refused(lib, pool((C.c_int32 * 2)(300, 6), need - 1), -2, f"< {need} bytes")                      # a small workspace
    # the embed entry without a handle, the cosine
    _refused(lib, lib.lds_xvector_embed(None, p, one, p, None, p, 1 << 16, 1, 20, None), -1, "null handle")
    _refused(lib, lib.lds_xvector_workspace_bytes(None, 1, 20, C.byref(nb)), -1, "null")
    _refused(lib, lib.lds_xvector_cosine(p, 0, p, 1, 8, p, None), -1, "N 0")
    _refused(lib, lib.lds_xvector_cosine(p, 1, p, 1, 0, p, None), -1, "dim 0")
    _refused(lib, lib.lds_xvector_cosine(p, 1, None, 1, 8, p, None), -1, "null")
    # the layer-sum entry checks its handle first
    _refused(lib, lib.lds_wavlm_encode_layersum(None, p, None, p, p, 0, p, 1 << 16, 1, 16000, None), -1, "null")


def test_python_refusals():
    from encoder.xvector import SpeakerEncoder, XVectorHead, equal_error_rate
    from lds import native
    st = head_state(768)
    with pytest.raises(ValueError, match="lacks .*tdnn.4.kernel.bias"):
        XVectorHead({k: v for k, v in st.items() if k != "tdnn.4.kernel.bias"})
    with pytest.raises(ValueError, match="no projector.weight"):
        XVectorHead({})
    with pytest.raises(ValueError, match="multiple of the K-step 32"):
        XVectorHead(head_state(48, geometry=None))
    with pytest.raises(ValueError, match="tdnn_dim\\[0\\] = 256"):
        XVectorHead(st, tdnn_dim=(256, 512, 512, 512, 1500))
    head = XVectorHead(st)
    assert (head.D, head.span, head.min_frames, head.n_labels, head.layer_weights) == (768, 14, 16, 512, None)
    with pytest.raises(RuntimeError, match="HIP device"):
        head.embed(torch.zeros(1, 20, 768))
    with pytest.raises(RuntimeError, match="HIP device"):
        SpeakerEncoder.similarity(torch.zeros(2, 8), torch.zeros(2, 8))
    summed = XVectorHead(head_state(768, 2))
    assert summed.layer_weights.shape == (3,) and abs(float(summed.layer_weights.sum()) - 1) < 1e-6 and np.ptp(summed.layer_weights) > 0.05
    # the binding's own checks (no device is touched)
    with pytest.raises(ValueError, match="1 .. 8 TDNN layers"):
        native.XVector(64, (), (), (), 32, {})
    with pytest.raises(ValueError, match="xvector_dim 30"):
        native.XVector(64, (64,), (1,), (1,), 30, {})
    assert abs(equal_error_rate([0.9, 0.8, 0.3, 0.1], [1, 1, 0, 0])) < 1e-12
    assert abs(equal_error_rate([0.9, 0.2, 0.3, 0.1], [1, 1, 0, 0]) - 0.5) < 1e-12
    with pytest.raises(ValueError, match="both"):
        equal_error_rate([0.5, 0.6], [1, 1])


class _FakeWavLMUnits:
    """what check_source and embed_audio look at"""
    hidden_dim = 768

    def __init__(self, n_layer=2, units_layer=None):
        from types import SimpleNamespace
        self.model = SimpleNamespace(dims={"n_layer": n_layer})
        self.units_layer = n_layer if units_layer is None else units_layer

    @staticmethod
    def frames_of(n):
        from lds import arch
        return arch.wavlm_frames(n)


_FakeWavLMUnits.__name__ = "WavLMUnits"


def test_check_source_and_short_clips():
    from encoder.xvector import SpeakerEncoder, XVectorHead
    last, summed = XVectorHead(head_state(768)), XVectorHead(head_state(768, 2))
    last.check_source(_FakeWavLMUnits())
    summed.check_source(_FakeWavLMUnits())
    with pytest.raises(ValueError, match="3 layer_weights against an encoder of 12 layers"):
        summed.check_source(_FakeWavLMUnits(12))
    with pytest.raises(ValueError, match=r"hidden_states\[1\]"):
        last.check_source(_FakeWavLMUnits(2, units_layer=1))
    wide = _FakeWavLMUnits()
    wide.hidden_dim = 1024
    with pytest.raises(ValueError, match="768-wide hidden states against a 1024-wide"):
        last.check_source(wide)
    spk = SpeakerEncoder(_FakeWavLMUnits(), last)
    with pytest.raises(RuntimeError, match="HIP device"):
        spk.embed_audio(torch.zeros(1, 16000))


def test_key_stripping_keeps_the_encoders_feature_extractor():
    """the head's top-level feature_extractor.{weight,bias} against the encoder's wavlm.feature_extractor.conv_layers.*: the prefix goes first"""
    from encoder.xvector import load_xvector_encoder_state
    sd = {"wavlm.feature_extractor.conv_layers.0.conv.weight": 1, "wavlm.feature_extractor.conv_layers.0.layer_norm.weight": 2,
          "wavlm.encoder.layer_norm.bias": 3, "wavlm.masked_spec_embed": 4,
          "feature_extractor.weight": 5, "feature_extractor.bias": 6, "projector.weight": 7, "tdnn.0.kernel.weight": 8, "classifier.bias": 9,
          "objective.weight": 10, "layer_weights": 11}
    out = load_xvector_encoder_state(sd)
    assert out == {"feature_extractor.conv_layers.0.conv.weight": 1, "feature_extractor.conv_layers.0.layer_norm.weight": 2, "encoder.layer_norm.bias": 3,
                   "masked_spec_embed": 4}
    with pytest.raises(ValueError, match="more than one encoder prefix"):
        load_xvector_encoder_state({"wavlm.a": 1, "hubert.b": 2})


def test_from_checkpoint(tmp_path):
    from encoder.xvector import XVectorHead
    geometry = dict(tdnn_dim=(64, 64, 96), tdnn_kernel=(3, 1, 1), tdnn_dilation=(2, 1, 1), xvector_output_dim=32)
    st = head_state(64, 2, geometry=geometry)
    sd = {k: torch.from_numpy(v) for k, v in st.items()}
    sd["wavlm.feature_extractor.conv_layers.0.conv.weight"] = torch.zeros(4, 1, 10)
    sd["objective.weight"] = torch.zeros(32, 2)
    torch.save(sd, tmp_path / "model.bin")
    json.dump(dict(geometry, use_weighted_layer_sum=True, hidden_size=64), open(tmp_path / "config.json", "w"))
    head = XVectorHead.from_checkpoint(tmp_path / "model.bin")
    assert (head.D, head.tdnn_dim, head.tdnn_kernel, head.tdnn_dilation, head.xvector_dim, head.span) == (64, (64, 64, 96), (3, 1, 1), (2, 1, 1), 32, 4)
    assert np.allclose(head.layer_weights, XN.softmax(st["layer_weights"]), atol=1e-7)
    assert "objective.weight" not in head._state and "layer_weights" not in head._state
    assert np.array_equal(head._state["feature_extractor.weight"], st["feature_extractor.weight"])
    # without the layer sum the stored weights are not used
    json.dump(dict(geometry, use_weighted_layer_sum=False), open(tmp_path / "config.json", "w"))
    assert XVectorHead.from_checkpoint(tmp_path / "model.bin").layer_weights is None
    # the flag without the tensor is refused; no config.json means the default geometry
    del sd["layer_weights"]
    torch.save(sd, tmp_path / "model.bin")
    json.dump(dict(geometry, use_weighted_layer_sum=True), open(tmp_path / "config.json", "w"))
    with pytest.raises(ValueError, match="holds no layer_weights"):
        XVectorHead.from_checkpoint(tmp_path / "model.bin")
    os.remove(tmp_path / "config.json")
    with pytest.raises(ValueError):
        XVectorHead.from_checkpoint(tmp_path / "model.bin")      # (64-wide tensors against the default geometry)
    torch.save({"lm_head.weight": torch.zeros(2, 2)}, tmp_path / "other.bin")
    with pytest.raises(ValueError, match="no projector.weight"):
        XVectorHead.from_checkpoint(tmp_path / "other.bin")


def test_binding_mirrors_the_header():
    """every new entry of include/lds.h / include/lds_test.h is declared once in lds.native, with as many arguments as the header has"""
    import re
    from conftest import ROOT
    from lds import native
    text = open(os.path.join(ROOT, "include", "lds.h")).read() + open(os.path.join(ROOT, "include", "lds_test.h")).read()
    names = [n for n in native.SIGNATURES if "xvector" in n or n == "lds_wavlm_encode_layersum"]
    assert len(names) == 10
    for n in names:
        m = re.search(r"\b" + n + r"\(([^;]*)\);", text)
        assert m, n
        args = [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]
        assert len(args) == len(native.SIGNATURES[n].partition(":")[2]), n
