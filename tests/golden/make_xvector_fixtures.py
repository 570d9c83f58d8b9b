"""Generate the x-vector head's golden fixtures from transformers' WavLMForXVector on the CPU.

Needs `transformers` (5.x) and torch; nothing is downloaded: the models are built from configs and filled with seeded weights.  Writes
(default: next to this script, `--out DIR` elsewhere):

  xvector.npz   three models, attn_implementation="eager", 2 layers, encoder weights from lds/arch.py wavlm_init_state (seed 0, loaded with
                strict=True), head weights from lds/arch.py xvector_init_state (uniform +- 1 / sqrt(fan_in), seed 0):
                    base_sum     WavLM-Base+ width, use_weighted_layer_sum=True (seeded, non-uniform layer_weights)
                    base_last    the same without the layer sum: the head reads last_hidden_state
                    large_last   WavLM-Large width (stable layer norm), every clip normalised to zero mean and unit variance first
                each on the four clips of tests/xvector_numpy.py (5,200 / 5,520 samples = 16 / 17 frames, and wavlm_numpy's clips of 75 and 350
                frames; regenerated from seeds, never stored), each clip ALONE with attention_mask=None, evaluated in float64:
                    m.embeddings   [4][512]      m.logits   [4][512]      m.cosine   [4][4] (F.cosine_similarity of every pair of embeddings)
                    m.absmax       [2]: the absmax of the embeddings and of the logits
                    m.gap          [2]: max |model fp32 - model fp64| / absmax, of the embeddings and of the logits
                    base_sum.hidden0   [16][768] float64: the head's input (the weighted layer sum) of the 16-frame clip, so that the CPU suite
                                   can run the float64 restatement (tests/xvector_numpy.py) without the encoder
                The generator asserts, for every model and clip, that the restatement on the model's own hidden states reproduces the model's
                embeddings and logits to 1e-12 x absmax.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_xvector_fixtures.py [--out DIR]
    python tests/golden/make_xvector_fixtures.py --check      # regenerate into a temporary directory, compare bit for bit
"""
import argparse
import importlib.util
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PKG = os.path.join(ROOT, "latent-diffusion-speech_amd")
FILES = ("xvector.npz",)
sys.dont_write_bytecode = True


def _load_by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def generate(out_dir):
    import torch
    from transformers import WavLMForXVector
    torch.manual_seed(0)
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    iw = _load_by_path("lds_init_weights", os.path.join(PKG, "lds", "init_weights.py"))
    arch = _load_by_path("lds_arch", os.path.join(PKG, "lds", "arch.py"))
    _load_by_path("hubert_numpy", os.path.join(ROOT, "tests", "hubert_numpy.py"))
    wnp = _load_by_path("wavlm_numpy", os.path.join(ROOT, "tests", "wavlm_numpy.py"))
    xn = _load_by_path("xvector_numpy", os.path.join(ROOT, "tests", "xvector_numpy.py"))
    gw = _load_by_path("make_wavlm_fixtures", os.path.join(HERE, "make_wavlm_fixtures.py"))
    clips = xn.make_clips(wnp, iw.uniform)

    out = {}
    for model in xn.MODELS:
        flavour, use_sum = model.split("_")[0], model.endswith("_sum")
        dims = wnp.dims_of(flavour, arch)
        w = arch.wavlm_init_state(dims, wnp.FIXTURE_SEED, init_weights=iw)
        sd = {"wavlm." + k: torch.from_numpy(v) for k, v in w.items()}
        sd["wavlm.masked_spec_embed"] = torch.from_numpy(iw.uniform("masked_spec_embed", (dims["n_state"],), wnp.FIXTURE_SEED, 0.0, 1.0))
        head = arch.xvector_init_state(dims["n_state"], xn.HEAD_SEED, dims["n_layer"] if use_sum else None, xn.N_LABELS, init_weights=iw)
        sd.update({k: torch.from_numpy(v) for k, v in head.items()})
        cfg = gw.config(flavour, wnp.FIXTURE_LAYERS)
        cfg.use_weighted_layer_sum = use_sum
        sd["objective.weight"] = torch.from_numpy(iw.uniform("xvector.objective.weight", (512, cfg.num_labels), xn.HEAD_SEED, -1.0, 1.0))      # (training only)
        assert tuple(cfg.tdnn_dim) == xn.DEFAULT["tdnn_dim"] and tuple(cfg.tdnn_kernel) == xn.DEFAULT["tdnn_kernel"]
        assert tuple(cfg.tdnn_dilation) == xn.DEFAULT["tdnn_dilation"] and cfg.xvector_output_dim == xn.DEFAULT["xvector_output_dim"]
        models = {}
        for dt in (torch.float32, torch.float64):
            m = WavLMForXVector(cfg)
            m.load_state_dict(sd, strict=True)
            models[dt] = m.to(dt).eval()
        emb, logit, gap = [], [], np.zeros(2)
        res32 = []
        for i, clip in enumerate(clips):
            wave = wnp.normalize_wave(clip, np.float64) if flavour == "large" else clip.astype(np.float64)
            with torch.no_grad():
                x64 = torch.from_numpy(wave)[None]
                o = models[torch.float64](x64, output_hidden_states=True)
                o32 = models[torch.float32](x64.float())
            hs = [h[0].numpy() for h in o.hidden_states]
            assert len(hs) == dims["n_layer"] + 1 and hs[0].shape[0] == xn.FRAMES[i] == arch.wavlm_frames(len(clip)), (model, i, hs[0].shape)
            hidden = xn.layer_sum(hs, head["layer_weights"]) if use_sum else hs[-1]
            e, z = xn.head(head, hidden)
            e_hf, z_hf = o.embeddings[0].numpy(), o.logits[0].numpy()
            # HF's logits of this model are the classifier's output, not cosine scores against `objective`
            assert np.abs(e - e_hf).max() <= 1e-12 * np.abs(e_hf).max(), (model, i, np.abs(e - e_hf).max())
            assert np.abs(z - z_hf).max() <= 1e-12 * np.abs(z_hf).max(), (model, i, np.abs(z - z_hf).max())
            emb.append(e_hf)
            logit.append(z_hf)
            res32.append((o32.embeddings[0].double().numpy(), o32.logits[0].double().numpy()))
            if model == "base_sum" and i == 0:
                out["base_sum.hidden0"] = hidden.astype(np.float64)
        emb, logit = np.stack(emb), np.stack(logit)
        am = np.array([np.abs(emb).max(), np.abs(logit).max()])
        for (e32, z32), e, z in zip(res32, emb, logit):
            gap = np.maximum(gap, [np.abs(e32 - e).max() / am[0], np.abs(z32 - z).max() / am[1]])
        cos = torch.nn.functional.cosine_similarity(torch.from_numpy(emb)[:, None, :], torch.from_numpy(emb)[None, :, :], dim=-1).numpy()
        assert np.abs(cos - xn.cosine(emb, emb)).max() < 1e-12
        out[f"{model}.embeddings"], out[f"{model}.logits"], out[f"{model}.cosine"] = emb, logit, cos
        out[f"{model}.absmax"], out[f"{model}.gap"] = am, gap
        off = cos[~np.eye(len(cos), dtype=bool)]
        print(f"{model}: embeddings absmax {am[0]:.4f}, logits absmax {am[1]:.4f}, fp32 gap {gap[0]:.2e} / {gap[1]:.2e}, "
              f"cosines between clips {off.min():.6f} .. {off.max():.6f}")
    np.savez_compressed(os.path.join(out_dir, FILES[0]), **out)
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
            a_, b_ = np.load(os.path.join(HERE, f)), np.load(os.path.join(tmp, f))
            assert sorted(a_.files) == sorted(b_.files), f
            for k in a_.files:
                assert a_[k].dtype == b_[k].dtype and a_[k].tobytes() == b_[k].tobytes(), (f, k)
    print("check ok: regenerated fixtures are bit-identical")


if __name__ == "__main__":
    main()
