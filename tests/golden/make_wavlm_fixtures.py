"""Generate the WavLM units encoder's golden fixtures from transformers.WavLMModel on the CPU.

Needs `transformers` (5.x) and torch; nothing is downloaded: the models are built from configs and filled with seeded weights.  Writes
(default: next to this script, `--out DIR` elsewhere):

  wavlm.npz             two models at full width with 2 layers, attn_implementation="eager", lds/arch.py wavlm_init_state(dims, seed 0) loaded with
                        strict=True (that proves the key naming):
                          base   WavLMConfig() (feat_extract_norm="group", do_stable_layer_norm=False; hidden 768, 12 heads, FFN 3072), the waveform as it is
                          large  WavLMConfig(feat_extract_norm="layer", do_stable_layer_norm=True, hidden_size=1024, num_attention_heads=16,
                                 intermediate_size=4096), every clip normalised first (Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm)
                        on six clips (tests/wavlm_numpy.py CLIPS: 400, 720, 24,240, 24,400, 112,240 and 288,400 samples = 1, 2, 75, 76, 350 and 901
                        frames; regenerated from seeds by make_clip, never stored).  Per flavour f and clip i: `f_rows_<i>` = the recorded frames
                        (hubert_numpy.fixture_rows: whole outputs would exceed the repository's file size limit) and, evaluated and stored in
                        float64, the rows of
                            f_feat_<i>   feature_extractor(wav) transposed (before the projection's LayerNorm)          [rows][512]
                            f_h1_<i>     hidden_states[1]                                                             [rows][hidden]
                            f_last_<i>   last_hidden_state                                                            [rows][hidden]
                        each with `f_gap_<name>_<i>` = max |model fp32 - model fp64| / absmax over the WHOLE output, and `f_absmax_<name>_<i>`;
                        `f_nobias_<i>` = max |last_hidden_state with rel_attn_embed zeroed - last_hidden_state| / absmax, and `f_gate_<i>` = (min, max)
                        of layer 0's gate over the recorded queries and all heads.
  manifest_wavlm.json   state-dict key -> shape of WavLMModel under the two configs at full depth (12 / 24 layers)

The generator asserts: every stage's abs-max lies in 0.1 .. 100; the frame rule; zeroing rel_attn_embed moves last_hidden_state by at least
100 x the GPU parity tolerance (2e-5 of abs-max) on every clip of more than one frame, so a wrong bias cannot pass; the gate spreads over at
least half of its range (1, 2) across the recorded queries of every clip of at least 75 frames.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_wavlm_fixtures.py [--out DIR]
    python tests/golden/make_wavlm_fixtures.py --check      # regenerate into a temporary directory, compare bit for bit
"""
import argparse
import importlib.util
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PKG = os.path.join(ROOT, "latent-diffusion-speech_amd")
FILES = ("manifest_wavlm.json", "wavlm.npz")
TOL = 2e-5      # the GPU suite's parity bound (tests/test_gpu_wavlm.py)
sys.dont_write_bytecode = True


def _load_by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def config(flavour, n_layer):
    from transformers import WavLMConfig
    if flavour == "large":
        return WavLMConfig(feat_extract_norm="layer", do_stable_layer_norm=True, hidden_size=1024, num_attention_heads=16, intermediate_size=4096,
                           num_hidden_layers=n_layer, attn_implementation="eager")
    return WavLMConfig(num_hidden_layers=n_layer, attn_implementation="eager")


def generate(out_dir):
    import torch
    from transformers import WavLMModel
    torch.manual_seed(0)
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    iw = _load_by_path("lds_init_weights", os.path.join(PKG, "lds", "init_weights.py"))
    arch = _load_by_path("lds_arch", os.path.join(PKG, "lds", "arch.py"))
    _load_by_path("hubert_numpy", os.path.join(ROOT, "tests", "hubert_numpy.py"))
    wnp = _load_by_path("wavlm_numpy", os.path.join(ROOT, "tests", "wavlm_numpy.py"))

    man = {}
    for fl, full in (("base+", 12), ("large", 24)):
        with torch.device("meta"):
            m = WavLMModel(config("large" if fl == "large" else "base", full))
        man[fl] = {k: list(v.shape) for k, v in m.state_dict().items()}
    with open(os.path.join(out_dir, FILES[0]), "w") as f:
        json.dump(man, f, indent=1, sort_keys=True)
        f.write("\n")

    out = {}
    for fl in wnp.FLAVOURS:
        dims = wnp.dims_of(fl, arch)
        w = arch.wavlm_init_state(dims, wnp.FIXTURE_SEED, init_weights=iw)
        sd = {k: torch.from_numpy(v) for k, v in w.items()}
        sd["masked_spec_embed"] = torch.from_numpy(iw.uniform("masked_spec_embed", (dims["n_state"],), wnp.FIXTURE_SEED, 0.0, 1.0))
        models = {}
        for dt in (torch.float32, torch.float64):
            m = WavLMModel(config(fl, wnp.FIXTURE_LAYERS))
            m.load_state_dict(sd, strict=True)
            models[dt] = m.to(dt).eval()
        sd0 = dict(sd)
        sd0["encoder.layers.0.attention.rel_attn_embed.weight"] = torch.zeros_like(sd["encoder.layers.0.attention.rel_attn_embed.weight"])
        nobias = WavLMModel(config(fl, wnp.FIXTURE_LAYERS))
        nobias.load_state_dict(sd0, strict=True)
        nobias = nobias.to(torch.float64).eval()
        for i in range(len(wnp.CLIPS)):
            clip = wnp.make_clip(i, iw.uniform)
            wave = wnp.normalize_wave(clip, np.float64) if fl == "large" else clip.astype(np.float64)
            res = {}
            for dt, m in models.items():
                with torch.no_grad():
                    x = torch.from_numpy(wave)[None].to(dt)
                    feat, o = m.feature_extractor(x).transpose(1, 2), m(x, output_hidden_states=True)
                res[dt] = {"feat": feat[0].double().numpy(), "h0": o.hidden_states[0][0].double().numpy(), "h1": o.hidden_states[1][0].double().numpy(),
                           "last": o.last_hidden_state[0].double().numpy()}
                assert np.array_equal(res[dt]["last"], o.hidden_states[wnp.FIXTURE_LAYERS][0].double().numpy())
            with torch.no_grad():
                nb = nobias(torch.from_numpy(wave)[None]).last_hidden_state[0].numpy()
            T = res[torch.float64]["last"].shape[0]
            assert T == wnp.FRAMES[i] == wnp.frames_of(len(clip)) == arch.wavlm_frames(len(clip)), (T, wnp.FRAMES[i])
            rows = wnp.fixture_rows(T, wnp.MAX_ROWS[i])
            out[f"{fl}_rows_{i}"] = rows
            for name in ("feat", "h1", "last"):
                r64, r32 = res[torch.float64][name], res[torch.float32][name]
                am = float(np.abs(r64).max())
                print(f"{fl} clip {i} ({len(clip)} samples, {T} frames) {name}: absmax {am:.3f}  fp32 gap {np.abs(r32 - r64).max() / am:.2e}")
                assert 0.1 < am < 100.0, (fl, i, name, am)
                out[f"{fl}_{name}_{i}"] = r64[rows].astype(np.float64)
                out[f"{fl}_gap_{name}_{i}"] = np.float64(np.abs(r32 - r64).max() / am)
                out[f"{fl}_absmax_{name}_{i}"] = np.float64(am)
            last = res[torch.float64]["last"]
            moved = float(np.abs(nb - last).max() / np.abs(last).max())
            # layer 0's gate from its attention input: hidden_states[0], behind the block's layer_norm in the stable flavour
            W = lambda k: w[k].astype(np.float64)      # noqa: E731
            h = res[torch.float64]["h0"]
            if dims["stable_layer_norm"]:
                h = wnp._layer_norm(h, W("encoder.layers.0.layer_norm.weight"), W("encoder.layers.0.layer_norm.bias"))
            g = wnp.gate_of(h, W("encoder.layers.0.attention.gru_rel_pos_linear.weight"), W("encoder.layers.0.attention.gru_rel_pos_linear.bias"),
                            W("encoder.layers.0.attention.gru_rel_pos_const"), dims["n_head"])[:, rows]
            print(f"{fl} clip {i}: zeroed rel_attn_embed moves last_hidden_state by {moved:.2e} of absmax; gate {g.min():.3f} .. {g.max():.3f}")
            if T > 1:
                assert moved >= 100 * TOL, (fl, i, moved)
            if T >= 75:
                assert g.max() - g.min() >= 0.5, (fl, i, float(g.min()), float(g.max()))
            out[f"{fl}_nobias_{i}"] = np.float64(moved)
            out[f"{fl}_gate_{i}"] = np.array([g.min(), g.max()], dtype=np.float64)
    np.savez_compressed(os.path.join(out_dir, FILES[1]), **out)
    for f in FILES:
        print(f, os.path.getsize(os.path.join(out_dir, f)), "bytes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    if not a.check:
        generate(a.out)
        return
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run([sys.executable, os.path.abspath(__file__), "--out", tmp], check=True, env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
        for f in FILES:
            if f.endswith(".npz"):
                a_, b_ = np.load(os.path.join(HERE, f)), np.load(os.path.join(tmp, f))
                assert sorted(a_.files) == sorted(b_.files), f
                for k in a_.files:
                    assert a_[k].dtype == b_[k].dtype and a_[k].tobytes() == b_[k].tobytes(), (f, k)
            else:
                assert open(os.path.join(HERE, f), "rb").read() == open(os.path.join(tmp, f), "rb").read(), f
    print("check ok: regenerated fixtures are bit-identical")


if __name__ == "__main__":
    main()
