"""Generate the XLSR-53 (wav2vec 2.0, layer-norm flavour) units encoder's golden fixtures from transformers.Wav2Vec2Model on the CPU.

Needs `transformers` (5.x) and torch; nothing is downloaded: the model is built from a config and filled with seeded weights.  Writes
(default: next to this script, `--out DIR` elsewhere):

  xlsr.npz             Wav2Vec2Model(Wav2Vec2Config(feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=True, hidden_size=1024,
                       num_hidden_layers=2, num_attention_heads=16, intermediate_size=4096, num_conv_pos_embeddings=128,
                       num_conv_pos_embedding_groups=16, attn_implementation="eager")) with lds/arch.py w2v_init_state(XLSR-53 widths,
                       2 layers, seed 0) loaded with strict=True through the key table (that proves the table), on five clips
                       (tests/w2v_numpy.py CLIPS: 400, 1,279, 41,277, 61,760 and 112,077 samples = 1, 3, 128, 192 and 349 frames;
                       regenerated from seeds by make_clip, never stored).  Per clip i: `rows_<i>` = the recorded frames
                       (hubert_numpy.fixture_rows: whole outputs of the long clips would exceed the repository's file size limit) and,
                       evaluated in float64 and stored rounded to float32, the rows of
                           feat_<i>   feature_extractor(wav) transposed (before the projection's LayerNorm)          [rows][512]
                           enc_<i>    last_hidden_state                                                              [rows][1024]
                       each with `gap_<name>_<i>` = max |model fp32 - model fp64| / absmax over the WHOLE output, and `absmax_<name>_<i>`.
  manifest_xlsr.json   the model's state-dict key -> shape under the config above with 24 layers, and the same under fairseq's names

The generator prints every stage's abs-max; all must lie in 0.1 .. 100 (asserted).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_xlsr_fixtures.py [--out DIR]
    python tests/golden/make_xlsr_fixtures.py --check      # regenerate into a temporary directory, compare bit for bit
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
FILES = ("manifest_xlsr.json", "xlsr.npz")
sys.dont_write_bytecode = True


def _load_by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def config(n_layer):
    from transformers import Wav2Vec2Config
    return Wav2Vec2Config(feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=True, hidden_size=1024, num_hidden_layers=n_layer,
                          num_attention_heads=16, intermediate_size=4096, num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16,
                          attn_implementation="eager")


def generate(out_dir):
    import torch
    from transformers import Wav2Vec2Model
    torch.manual_seed(0)
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    iw = _load_by_path("lds_init_weights", os.path.join(PKG, "lds", "init_weights.py"))
    arch = _load_by_path("lds_arch", os.path.join(PKG, "lds", "arch.py"))
    _load_by_path("hubert_numpy", os.path.join(ROOT, "tests", "hubert_numpy.py"))
    wnp = _load_by_path("w2v_numpy", os.path.join(ROOT, "tests", "w2v_numpy.py"))

    with torch.device("meta"):
        full = Wav2Vec2Model(config(24))
    man = {"transformers": {k: list(v.shape) for k, v in full.state_dict().items()},
           "fairseq": {k: list(s) for k, s in arch.w2v_param_shapes(arch.XLSR_53_DIMS).items()}}
    with open(os.path.join(out_dir, FILES[0]), "w") as f:
        json.dump(man, f, indent=1, sort_keys=True)
        f.write("\n")

    dims = dict(arch.XLSR_53_DIMS, n_layer=wnp.FIXTURE_LAYERS)
    w = arch.w2v_init_state(dims, wnp.FIXTURE_SEED, init_weights=iw)
    sd = {arch.w2v_key_to_transformers(k): torch.from_numpy(v) for k, v in w.items()}
    sd["masked_spec_embed"] = torch.from_numpy(iw.uniform("mask_emb", (dims["n_state"],), wnp.FIXTURE_SEED, 0.0, 1.0))
    models = {}
    for dt in (torch.float32, torch.float64):
        m = Wav2Vec2Model(config(wnp.FIXTURE_LAYERS))
        m.load_state_dict(sd, strict=True)
        models[dt] = m.to(dt).eval()

    out = {}
    for i in range(len(wnp.CLIPS)):
        clip = wnp.make_clip(i, iw.uniform)
        res = {}
        for dt, m in models.items():
            with torch.no_grad():
                x = torch.from_numpy(clip)[None].to(dt)
                # (the model's own `extract_features` output is already normalised by the projection's LayerNorm: the extractor is called itself)
                feat, o = m.feature_extractor(x).transpose(1, 2), m(x)
            res[dt] = {"feat": feat[0].double().numpy(), "enc": o.last_hidden_state[0].double().numpy()}
        T = res[torch.float64]["enc"].shape[0]
        assert T == wnp.FRAMES[i] == wnp.frames_of(len(clip)), (T, wnp.FRAMES[i])
        rows = wnp.fixture_rows(T, wnp.MAX_ROWS[i])
        out[f"rows_{i}"] = rows
        for name in ("feat", "enc"):
            r64, r32 = res[torch.float64][name], res[torch.float32][name]
            am = float(np.abs(r64).max())
            print(f"clip {i} ({len(clip)} samples, {T} frames) {name}: absmax {am:.3f}  fp32 gap {np.abs(r32 - r64).max() / am:.2e}")
            assert 0.1 < am < 100.0, (i, name, am)
            out[f"{name}_{i}"] = r64[rows].astype(np.float32)
            out[f"gap_{name}_{i}"] = np.float64(np.abs(r32 - r64).max() / am)
            out[f"absmax_{name}_{i}"] = np.float64(am)
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
