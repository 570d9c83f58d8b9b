"""Generate the w2v-BERT 2.0 units encoder's golden fixtures from transformers' Wav2Vec2BertModel and SeamlessM4TFeatureExtractor on the CPU.

Needs `transformers` (5.x) and torch; nothing is downloaded: the model is built from a config and filled with seeded weights, the feature
extractor from its defaults.  Writes (default: next to this script, `--out DIR` elsewhere):

  w2vbert.npz             Wav2Vec2BertModel(Wav2Vec2BertConfig(num_hidden_layers=2, attn_implementation="eager")) at full width with
                          lds/arch.py w2vbert_init_state(2 layers, seed 0) loaded with strict=True (that proves the naming), run in float64 on
                          SeamlessM4TFeatureExtractor()(clip as a numpy array, sampling_rate=16000) as the reference runs it, on five clips
                          (tests/w2vbert_numpy.py CLIPS: 560, 720, 24,240, 24,400 and 64,240 samples = 2, 3, 150, 151 and 400 frames = 1, 2, 75,
                          76 and 200 rows; regenerated from seeds by make_clip, never stored).  Per clip i: `rows_<i>` = the recorded rows
                          (hubert_numpy.fixture_rows: whole outputs of the long clips would exceed the repository's file size limit) and
                              feats_<i>   the extractor's input_features (float32 as it returns them)            [rows][160]
                              enc_<i>     last_hidden_state in float64, stored rounded to float32                  [rows][1024]
                          with `gap_feats_<i>` = max |extractor - float64 restatement (tests/w2vbert_numpy.py fbank)| / absmax and
                          `gap_enc_<i>` = max |model fp32 - model fp64| / absmax, both over the WHOLE output, and `absmax_<name>_<i>`.
  manifest_w2vbert.json   the model's state-dict key -> shape under Wav2Vec2BertConfig() (24 layers)

The generator asserts every stage's abs-max in 0.1 .. 100, every per-bin standard deviation of the log-mel above 0.05, the frame rule, and that
the float64 restatement of the model agrees with transformers' float64 model to 1e-9 of absmax.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_w2vbert_fixtures.py [--out DIR]
    python tests/golden/make_w2vbert_fixtures.py --check      # regenerate into a temporary directory: arrays bit for bit, the absmax_* / gap_* scalars to 1e-12 / 1e-6 of themselves
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
FILES = ("manifest_w2vbert.json", "w2vbert.npz")
sys.dont_write_bytecode = True


def _load_by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def config(n_layer):
    from transformers import Wav2Vec2BertConfig
    return Wav2Vec2BertConfig(num_hidden_layers=n_layer, attn_implementation="eager")


def generate(out_dir):
    import torch
    from transformers import SeamlessM4TFeatureExtractor, Wav2Vec2BertModel
    torch.manual_seed(0)
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    iw = _load_by_path("lds_init_weights", os.path.join(PKG, "lds", "init_weights.py"))
    arch = _load_by_path("lds_arch", os.path.join(PKG, "lds", "arch.py"))
    _load_by_path("hubert_numpy", os.path.join(ROOT, "tests", "hubert_numpy.py"))
    wnp = _load_by_path("w2vbert_numpy", os.path.join(ROOT, "tests", "w2vbert_numpy.py"))

    with torch.device("meta"):
        full = Wav2Vec2BertModel(config(24))
    with open(os.path.join(out_dir, FILES[0]), "w") as f:
        json.dump({"transformers": {k: list(v.shape) for k, v in full.state_dict().items()}}, f, indent=1, sort_keys=True)
        f.write("\n")

    dims = dict(arch.W2V_BERT_DIMS, n_layer=wnp.FIXTURE_LAYERS)
    w = arch.w2vbert_init_state(dims, wnp.FIXTURE_SEED, init_weights=iw)
    sd = {k: torch.from_numpy(v) for k, v in w.items()}
    sd["masked_spec_embed"] = torch.from_numpy(iw.uniform("masked_spec_embed", (dims["n_state"],), wnp.FIXTURE_SEED, 0.0, 1.0))
    models = {}
    for dt in (torch.float32, torch.float64):
        m = Wav2Vec2BertModel(config(wnp.FIXTURE_LAYERS))
        m.load_state_dict(sd, strict=True)
        models[dt] = m.to(dt).eval()
    fe = SeamlessM4TFeatureExtractor()

    out = {}
    for i in range(len(wnp.CLIPS)):
        clip = wnp.make_clip(i, iw.uniform)
        n, valid, rows_n = wnp.frames_of(len(clip))
        assert (n, rows_n) == (wnp.FRAMES[i], wnp.ROWS[i]) and arch.w2vbert_frames(len(clip)) == (n, valid, rows_n)
        inp = fe(clip, sampling_rate=16000, return_tensors="pt")
        feats, mask = inp["input_features"], inp["attention_mask"]
        assert tuple(feats.shape) == (1, rows_n, 160) and int(mask.sum()) == valid and bool((mask[0, :valid] == 1).all()), (feats.shape, mask)
        std = wnp.log_mel(clip).std(axis=0, ddof=1)
        assert std.min() > 0.05, (i, float(std.min()))
        res = {}
        for dt, m in models.items():
            with torch.no_grad():
                res[dt] = m(input_features=feats.to(dt), attention_mask=mask).last_hidden_state[0].double().numpy()
        f64 = wnp.fbank(clip)
        f32 = feats[0].double().numpy()
        e64 = res[torch.float64]
        re = wnp.encode(w, dims, feats[0].numpy(), n, np.float64)
        agree = float(np.abs(re - e64).max() / np.abs(e64).max())
        assert agree < 1e-9, (i, agree)
        rows = wnp.fixture_rows(rows_n, wnp.MAX_ROWS[i])
        out[f"rows_{i}"] = rows
        for name, r64, r32, store in (("feats", f64, f32, feats[0].numpy()), ("enc", e64, res[torch.float32], e64.astype(np.float32))):
            am = float(np.abs(r64).max())
            print(f"clip {i} ({len(clip)} samples, {n} frames, {rows_n} rows) {name}: absmax {am:.3f}  fp32 gap {np.abs(r32 - r64).max() / am:.2e}"
                  f"  min log-mel std {std.min():.3f}  restatement vs fp64 model {agree:.1e}")
            assert 0.1 < am < 100.0, (i, name, am)
            out[f"{name}_{i}"] = np.ascontiguousarray(store[rows]).astype(np.float32)
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
                    assert a_[k].dtype == b_[k].dtype, (f, k)
                    if k.startswith(("gap_", "absmax_")):
                        # float64 scalars out of numpy reductions: their last bits depend on the host's numpy / BLAS threads (2e-15 absolute).
                        # A gap is such a difference over absmax (~1e-6), so the same 2e-15 is 2e-9 of it
                        assert np.allclose(a_[k], b_[k], rtol=1e-6 if k.startswith("gap_") else 1e-12, atol=0.0), (f, k, a_[k], b_[k])
                    else:
                        assert a_[k].tobytes() == b_[k].tobytes(), (f, k)
            else:
                assert open(os.path.join(HERE, f), "rb").read() == open(os.path.join(tmp, f), "rb").read(), f
    print("check ok: regenerated arrays are bit-identical, the recorded gaps agree")


if __name__ == "__main__":
    main()
