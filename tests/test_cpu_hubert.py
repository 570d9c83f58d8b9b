"""The HuBERT units encoder (encoder.hubert.model, tools.tools.HubertUnits / Units_Encoder, include/lds.h lds_hubert_*) without a GPU:
the numpy restatement the GPU tests lean on (pinned to the fixtures recorded from the reference), the frame rule, the parameter
enumeration and public signatures, the weight-norm fold, the exported symbols, and the argument validation, which must refuse before a
device is touched."""
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import hubert_numpy as hnp
from conftest import GOLDEN, PKG, ROOT


def _manifest():
    return json.load(open(os.path.join(GOLDEN, "manifest_hubert.json")))


@pytest.fixture(scope="module")
def weights():
    from lds import arch
    return arch.hubert_init_state(arch.HUBERT_BASE_DIMS, hnp.FIXTURE_SEED)


@pytest.mark.parametrize("clip", [0, 1, 2, 3, 4])
def test_numpy_restatement_reproduces_the_reference(clip, weights):
    """float64 mode within 1e-6 absmax of the fixtures (they hold the reference's float64 result rounded to float32); float32 mode within
    twice the reference's own fp32-against-fp64 gap of that output.  The feature extractor, layers 0 and 2 of all five clips, and for the
    two shortest clips the 12-layer output and the units."""
    from lds import arch, init_weights
    z = np.load(os.path.join(GOLDEN, "hubert.npz"))
    audio = hnp.make_clip(clip, init_weights.uniform)
    rows = z[f"rows_{clip}"]
    names = [("feat", None, False), ("l0", 0, False), ("l2", 2, False)] + ([("l12", None, False), ("units", None, True)] if clip < 2 else [])
    for dtype, bound in ((np.float64, None), (np.float32, 2.0)):
        feats = hnp.features(weights, audio, dtype)
        for name, layer, proj in names:
            got = feats if name == "feat" else hnp.encode(weights, arch.HUBERT_BASE_DIMS, audio, layer=layer, proj=proj, dtype=dtype, feats=feats)
            assert got.dtype == dtype and got.shape[0] == hnp.CLIPS[clip][0] // 320
            e = np.abs(got[rows].astype(np.float64) - z[f"{name}_{clip}"]).max() / float(z[f"absmax_{name}_{clip}"])
            tol = 1e-6 if bound is None else bound * float(z[f"gap_{name}_{clip}"])
            print(f"clip {clip} {name} {dtype.__name__}: {e:.2e} (bound {tol:.2e})")
            assert e <= tol, (name, dtype.__name__, e, tol)


def test_fixture_stages_live_at_a_scale_of_order_one():
    z = np.load(os.path.join(GOLDEN, "hubert.npz"))
    am = [float(z[k]) for k in z.files if k.startswith("absmax_")]
    assert len(am) == 21 and min(am) >= 0.1 and max(am) <= 100.0
    gaps = [float(z[k]) for k in z.files if k.startswith("gap_")]
    assert max(gaps) < 2e-5 / 10      # the project's bound leaves an order of magnitude over the reference's own fp32 error


def test_frame_rule_is_floor_division_by_320():
    from lds import arch, native
    for L in list(range(320, 4000)) + [41277, 61760, 112077, 479999, 480000]:
        assert arch.hubert_frames(L) == hnp.frames_of(L) == native.Hubert.frames(L) == L // 320, L
    assert hnp.level_frames(1279) == [270, 134, 66, 32, 15, 7, 3] and hnp.level_frames(320)[0] == 79
    assert arch.hubert_frames(400, pad=0) == 1 and arch.hubert_frames(16000, pad=0) == 49      # Hubert.encode on a waveform as given


def test_param_shapes_and_state_dict_keys_equal_the_reference():
    from encoder.hubert.model import HubertDiscrete, HubertSoft
    from lds import arch
    man = _manifest()
    assert man["base_dims"] == arch.HUBERT_BASE_DIMS
    for name, cls, n_label in (("soft", HubertSoft, 100), ("discrete", lambda: HubertDiscrete(None), 504)):
        shapes = arch.hubert_param_shapes(arch.HUBERT_BASE_DIMS, n_label)
        assert list(shapes) == list(man[name]) and all(list(shapes[k]) == man[name][k] for k in shapes), name
        sd = cls().state_dict()
        assert list(sd) == list(man[name]) and all(list(sd[k].shape) == man[name][k] for k in sd), name
    assert len(man["soft"]) == 166 and abs(sum(int(np.prod(s)) for s in man["soft"].values()) - 94.6e6) < 0.1e6
    state = arch.hubert_init_state(arch.HUBERT_BASE_DIMS, 0)
    m = HubertSoft()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    assert arch.get_encoder_out_channels("hubertsoft") == 256 and arch.get_encoder_out_channels("contentvec768l12") == 768


def test_public_signatures_equal_the_reference():
    from encoder.hubert import model as M
    sig = _manifest()["signatures"]

    def same(ref, fn):
        """the reference's parameters, in order, with their defaults and annotations; keyword-only extensions may follow"""
        got = str(inspect.signature(fn))
        ref_params = ref[1:ref.rindex(")")]
        return got.startswith("(" + ref_params) and (got[1 + len(ref_params)] in ",)") and got.endswith(ref[ref.rindex(")"):])
    for name, fn in (("Hubert.__init__", M.Hubert.__init__), ("Hubert.encode", M.Hubert.encode), ("Hubert.forward", M.Hubert.forward),
                     ("Hubert.logits", M.Hubert.logits), ("Hubert.mask", M.Hubert.mask), ("HubertSoft.__init__", M.HubertSoft.__init__),
                     ("HubertSoft.units", M.HubertSoft.units), ("HubertDiscrete.__init__", M.HubertDiscrete.__init__),
                     ("HubertDiscrete.units", M.HubertDiscrete.units), ("hubert_soft", M.hubert_soft), ("hubert_discrete", M.hubert_discrete)):
        assert same(sig[name], fn), (name, sig[name], str(inspect.signature(fn)))


def test_weight_norm_fold_equals_torch_parametrization():
    from lds import arch, init_weights
    conv = torch.nn.Conv1d(32, 32, kernel_size=8, padding=4, groups=2)
    conv = torch.nn.utils.parametrizations.weight_norm(conv, name="weight", dim=2)
    g = init_weights.uniform("t.g", (1, 1, 8), 3, 1.5, 3.0)
    v = init_weights.uniform("t.v", (32, 16, 8), 3, -0.3, 0.3)
    with torch.no_grad():
        conv.parametrizations.weight.original0.copy_(torch.from_numpy(g))
        conv.parametrizations.weight.original1.copy_(torch.from_numpy(v))
        conv = conv.double()
        ref = conv.weight.numpy()
    for fold in (arch.hubert_fold_weight_norm, hnp.fold_weight_norm):
        got = fold(g, v)
        assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-14 * np.abs(ref).max() + 1e-16


def test_symbols_declared_once_and_exported():
    from lds import native
    names = ("lds_hubert_create", "lds_hubert_destroy", "lds_hubert_workspace_bytes", "lds_hubert_features", "lds_hubert_encode")
    header = open(os.path.join(ROOT, "include", "lds.h")).read()
    table = open(os.path.join(PKG, "lds", "native.py")).read()
    for n in names:
        assert len(re.findall(rf"\b{n}\(", header)) == 1, n
        assert len(re.findall(rf"^{n}\s", table, flags=re.M)) == 1 and n in native.EXPORTS, n
        assert hasattr(native.lib(), n), n
    body = re.search(r"typedef\s+struct\s+lds_hubert_cfg\s*\{\s*int([^}]*);\s*\}\s*lds_hubert_cfg\s*;", header)      # the binding mirrors the struct
    assert body and [f.strip() for f in body.group(1).split(",")] == [f for f, _ in native.HubertCfg._fields_] == list(native.Hubert.FIELDS)
    import ctypes
    assert all(t is ctypes.c_int for _, t in native.HubertCfg._fields_)
    assert "hubert.hip" in open(os.path.join(PKG, "csrc", "Makefile")).read()


@pytest.mark.parametrize("change, match", [
    (dict(conv_dim=500), "conv_dim"), (dict(n_state=800, n_head=12), "n_state"), (dict(n_head=8), "64 \\* n_head"),
    (dict(pos_groups=32), "pos_groups"), (dict(pos_groups=7), "pos_groups"), (dict(pos_kernel=127), "pos_kernel"), (dict(pos_kernel=130), "pos_kernel"),
    (dict(n_layer=0), "n_layer"), (dict(n_ctx=1501), "n_ctx"), (dict(n_ffn=100), "n_ffn"), (dict(n_proj=0), "n_proj")])
def test_bad_dimensions_are_value_errors(change, match):
    from encoder.hubert.model import HubertSoft
    from lds import arch, native
    dims = dict(arch.HUBERT_BASE_DIMS, **change)
    with pytest.raises(ValueError, match=match):
        native.Hubert.check_dims(dims)
    with pytest.raises(ValueError, match=match):
        HubertSoft(dims=dims)


class _NoDevice:
    """a native.Hubert whose limits can be asked without a handle"""

    def __init__(self):
        from lds import arch, native
        self.h = native.Hubert.__new__(native.Hubert)
        self.h.dims = dict(arch.HUBERT_BASE_DIMS, n_layer=2)


def test_call_limits_are_value_errors_before_a_device_is_touched():
    h = _NoDevice().h
    cpu = torch.zeros(2, 16000)
    with pytest.raises(ValueError, match="at least 320 samples"):
        h.encode(torch.zeros(1, 319))
    with pytest.raises(ValueError, match="more than n_ctx 1500"):
        h.encode(torch.zeros(1, 480320))
    with pytest.raises(ValueError, match="lengths must be 2 integers in 320 .. 16000"):
        h.encode(cpu, [319, 16000])
    with pytest.raises(ValueError, match="lengths must be 2 integers in 320 .. 16000"):
        h.features(cpu, [16000, 16001])
    with pytest.raises(ValueError, match="at most 64 clips"):
        h.encode(torch.zeros(65, 16000), [16000] * 65)
    with pytest.raises(ValueError, match="layer 3 outside 0 .. 2"):
        h.encode(cpu, layer=3)
    with pytest.raises(ValueError, match="layer -1 outside"):
        h.encode(cpu, layer=-1)
    with pytest.raises(ValueError, match="proj follows the last layer"):
        h.encode(cpu, layer=1, proj=True)
    with pytest.raises(ValueError, match="pad 41"):
        h.encode(cpu, pad=41)
    with pytest.raises(ValueError, match=r"must be \[B, L\]"):
        h.encode(torch.zeros(16000))
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # everything valid: the CPU tensor is what is refused
        h.encode(cpu, [16000, 320])


def test_cpu_tensors_and_the_training_path_raise():
    from encoder.hubert.model import Hubert, HubertDiscrete, HubertSoft
    m = HubertSoft()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.units(torch.zeros(1, 1, 16000))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.encode(torch.zeros(1, 1, 16000), layer=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.units_ragged(torch.zeros(2, 16000), [16000, 400])
    with pytest.raises(ValueError, match="lengths must be"):
        m.units_ragged(torch.zeros(2, 16000), [16000, 100])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HubertDiscrete(object()).units(torch.zeros(1, 1, 16000))
    for fn in (Hubert().forward, Hubert().logits, Hubert().mask):
        with pytest.raises(NotImplementedError, match="training path"):
            fn(torch.zeros(1, 1, 16000))


def test_pretrained_raises_without_any_attempt_to_fetch(monkeypatch):
    from encoder.hubert import model as M

    def no_network(*a, **k):
        raise AssertionError("a download was attempted")
    monkeypatch.setattr(torch.hub, "load_state_dict_from_url", no_network)
    monkeypatch.setattr(torch.hub, "download_url_to_file", no_network)
    for fn in (M.hubert_soft, M.hubert_discrete):
        with pytest.raises(NotImplementedError, match="checkpoint=PATH"):
            fn()
        with pytest.raises(NotImplementedError, match="checkpoint=PATH"):
            fn(pretrained=True, progress=False)
    assert isinstance(M.hubert_soft(pretrained=False), M.HubertSoft) and isinstance(M.hubert_discrete(False), M.HubertDiscrete)
    assert "checkpoint" in inspect.signature(M.hubert_soft).parameters
    assert inspect.signature(M.hubert_soft).parameters["checkpoint"].kind is inspect.Parameter.KEYWORD_ONLY


def test_a_local_checkpoint_loads_strictly(tmp_path, weights):
    from encoder.hubert import model as M
    from tools.tools import HubertUnits, Units_Encoder
    path = tmp_path / "hubert-soft.pt"
    torch.save({"module." + k: torch.from_numpy(v) for k, v in weights.items()}, path)
    m = M.hubert_soft(checkpoint=str(path))
    assert torch.equal(m.state_dict()["proj.weight"], torch.from_numpy(weights["proj.weight"]))
    enc = Units_Encoder("contentvec768l12", device="cpu", checkpoint=str(path))
    assert isinstance(enc.model, HubertUnits) and enc.model.hidden_dim == 768 and enc.min_samples == 320
    bad = dict(weights)
    del bad["masked_spec_embed"]
    torch.save({k: torch.from_numpy(v) for k, v in bad.items()}, path)
    with pytest.raises(RuntimeError, match="masked_spec_embed"):
        M.hubert_soft(checkpoint=str(path))


def test_units_encoder_names():
    from lds import arch
    from tools.tools import HubertUnits, Units_Encoder
    dims = dict(arch.HUBERT_BASE_DIMS, n_layer=1)
    for name, width in (("hubertsoft", 256), ("contentvec768l12", 768)):
        with pytest.raises(ValueError, match="needs checkpoint=PATH"):
            Units_Encoder(name, device="cpu")
        enc = Units_Encoder(name, device="cpu", model=HubertUnits.synthetic(name, dims, device="cpu"))
        assert enc.model.hidden_dim == width == arch.get_encoder_out_channels(name) and enc.min_samples == 320
        assert enc.model.frames_of(112077) == 350 and enc.model.n_ctx == 1500
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            enc.encode(torch.zeros(16000), 16000)
        with pytest.raises(ValueError, match="lengths must be 2 integers in 320 .. 16000"):
            enc.model.encode_ragged(torch.zeros(2, 16000), [16000, 319])      # (the lengths are judged before the device)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            enc.model.encode_ragged(torch.zeros(2, 16000), [16000, 320])
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            enc.encode_ragged(torch.zeros(2, 16000), [16000, 320])
    with pytest.raises(ValueError, match="Unknown units encoder"):
        Units_Encoder("contentvec")
    with pytest.raises(ValueError, match="Unknown units encoder"):
        HubertUnits("whisper_large_v3", dims=dims, state={})
    with pytest.raises(NotImplementedError, match="w2v-bert"):
        Units_Encoder("w2v-bert")
    with pytest.raises(NotImplementedError, match="xlsr_53_56k"):
        Units_Encoder("xlsr_53_56k")


def test_plan_long_audio_takes_the_frame_rule_from_the_encoder():
    from encoder.whisper.model import ModelDimensions
    from lds import arch
    from tools.infer_tools import DiffusionSVC
    from tools.tools import HubertUnits, Units_Encoder, WhisperLargeV3
    ranges = [(0, 0, 30000), (170, 31000, 31500), (180, 33000, 63000), (400, 70000, 78000)]
    svc = DiffusionSVC(device="cpu")
    svc.args = {"data": {"block_size": 512, "sampling_rate": 44100}}
    svc.units_encoder = Units_Encoder("hubertsoft", device="cpu", resample=True,
                                      model=HubertUnits.synthetic("hubertsoft", dict(arch.HUBERT_BASE_DIMS, n_layer=1), device="cpu"))
    plan = svc._plan_long_audio(44100, ranges, batch_size=3)
    assert plan["hop_size"] == 512.0 and plan["n_frames"] == [59, 1, 59, 16] and plan["chunks"] == [[1, 3, 0], [2]]
    # 30 s at 16 kHz = 480,000 samples = 1500 frames: the window; 320 samples more is one frame too many.  Whisper's rule gives 1500
    # frames up to 480,319 samples as well, but counts (L // 160 - 1) // 2 + 1, so the two differ on 480,160 samples
    ok = -(-480000 * 44100 // 16000)
    svc._plan_long_audio(44100, [(0, 0, ok)], batch_size=1)
    with pytest.raises(ValueError, match=r"segment 0 .*exceeds the units encoder's window of 1500 frames \(30 s for HuBERT\)"):
        svc._plan_long_audio(16000, [(0, 0, 480320)], batch_size=1)
    svc._plan_long_audio(16000, [(0, 0, 480319)], batch_size=1)
    dims = ModelDimensions(**dict(arch.WHISPER_LARGE_V3_DIMS, n_audio_state=64, n_audio_head=1, n_audio_layer=1))
    svc.units_encoder = Units_Encoder("whisper_large_v3", device="cpu", model=WhisperLargeV3.synthetic(dims, device="cpu"), resample=True)
    assert svc._plan_long_audio(44100, ranges, batch_size=3) == plan      # the Whisper plan is what it was
    svc._plan_long_audio(16000, [(0, 0, 480159)], batch_size=1)
    with pytest.raises(ValueError, match=r"exceeds the units encoder's window of 1500 frames \(30 s for Whisper\)"):
        svc._plan_long_audio(16000, [(0, 0, 480160)], batch_size=1)
