"""Generate the CTC heads' golden fixtures from transformers' Wav2Vec2ForCTC and WavLMForCTC on the CPU.

Needs `transformers` (5.x) and torch; nothing is downloaded: the models are built from configs and filled with seeded weights.  Writes
(default: next to this script, `--out DIR` elsewhere):

  ctc.npz   two models, attn_implementation="eager", encoder weights from the existing seeded initialisers through the existing key tables
            (lds/arch.py w2v_init_state / wavlm_init_state, seed 0, 2 layers, loaded with strict=True), lm_head from lds/init_weights.py
            (uniform +- 1 / sqrt(D): encoder.ctc.CTCHead.synthetic(D, V, seed 0)):
                xlsr    Wav2Vec2ForCTC(make_xlsr_fixtures.config(2), vocab_size=32, pad_token_id=0)
                wavlm   WavLMForCTC(make_wavlm_fixtures' base config, vocab_size=33, pad_token_id=0)
            on tests/w2v_numpy.py CLIPS 1 and 2 (1,279 and 41,277 samples = 3 and 128 frames; regenerated from seeds, never stored).
            Per model m and clip i, evaluated in float64 and stored rounded to float32 where a float array:
                m.clip<i>.logprobs      logits.log_softmax(-1)                                             [T][V]
                m.clip<i>.ids           logits.argmax(-1)                                                  [T]
                m.clip<i>.greedy        those ids with runs collapsed and the blank dropped
                m.clip<i>.inside        frames whose float64 top-2 logit gap is below 2 delta_z (tests/ctc_numpy.py): the native head is held
                                        to the criterion there, not to id equality
                m.clip<i>.labels<L>     seeded labels of length L = 0, 1, 40 (ids 1 .. V - 1)
                m.clip<i>.loss<L>       F.ctc_loss(reduction="sum") of the float64 log-probs, float64 (+inf where the labels do not fit)
                m.clip<i>.hfloss<L>     the model's own .loss (ctc_loss_reduction="sum"); transformers casts the log-probs to fp32 first
                m.clip<i>.gap           max |model fp32 - model fp64| of the log-probs / their absmax;  m.clip<i>.absmax
            The generator asserts that at most 1 % of all frames are `inside`, and that the two losses agree within bound 3.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_ctc_fixtures.py [--out DIR]
    python tests/golden/make_ctc_fixtures.py --check      # regenerate into a temporary directory, compare bit for bit
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
FILES = ("ctc.npz",)
CLIPS = (1, 2)
LABEL_LENGTHS = (0, 1, 40)
VOCAB = {"xlsr": 32, "wavlm": 33}
SEED = 0
sys.dont_write_bytecode = True


def _load_by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def head_weights(iw, D, V):
    k = 1.0 / np.sqrt(D)
    return iw.uniform("lm_head.weight", (V, D), SEED, -k, k), iw.uniform("lm_head.bias", (V,), SEED, -k, k)


def labels_of(iw, model, clip, L, V):
    u = iw.uniform(f"ctc.labels.{model}.{clip}.{L}", (L,), SEED, 0.0, 1.0)
    return np.minimum(1 + np.floor(u.astype(np.float64) * (V - 1)), V - 1).astype(np.int64)


def generate(out_dir):
    import torch
    from transformers import Wav2Vec2ForCTC, WavLMForCTC
    torch.manual_seed(0)
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    iw = _load_by_path("lds_init_weights", os.path.join(PKG, "lds", "init_weights.py"))
    arch = _load_by_path("lds_arch", os.path.join(PKG, "lds", "arch.py"))
    _load_by_path("hubert_numpy", os.path.join(ROOT, "tests", "hubert_numpy.py"))
    wnp = _load_by_path("w2v_numpy", os.path.join(ROOT, "tests", "w2v_numpy.py"))
    lnp = _load_by_path("wavlm_numpy", os.path.join(ROOT, "tests", "wavlm_numpy.py"))
    cn = _load_by_path("ctc_numpy", os.path.join(ROOT, "tests", "ctc_numpy.py"))
    gx = _load_by_path("make_xlsr_fixtures", os.path.join(HERE, "make_xlsr_fixtures.py"))
    gw = _load_by_path("make_wavlm_fixtures", os.path.join(HERE, "make_wavlm_fixtures.py"))

    def build(model):
        V = VOCAB[model]
        if model == "xlsr":
            dims = dict(arch.XLSR_53_DIMS, n_layer=wnp.FIXTURE_LAYERS)
            w = arch.w2v_init_state(dims, wnp.FIXTURE_SEED, init_weights=iw)
            sd = {"wav2vec2." + arch.w2v_key_to_transformers(k): torch.from_numpy(v) for k, v in w.items()}
            sd["wav2vec2.masked_spec_embed"] = torch.from_numpy(iw.uniform("mask_emb", (dims["n_state"],), wnp.FIXTURE_SEED, 0.0, 1.0))
            cfg, cls = gx.config(wnp.FIXTURE_LAYERS), Wav2Vec2ForCTC
        else:
            dims = lnp.dims_of("base", arch)
            w = arch.wavlm_init_state(dims, lnp.FIXTURE_SEED, init_weights=iw)
            sd = {"wavlm." + k: torch.from_numpy(v) for k, v in w.items()}
            sd["wavlm.masked_spec_embed"] = torch.from_numpy(iw.uniform("masked_spec_embed", (dims["n_state"],), lnp.FIXTURE_SEED, 0.0, 1.0))
            cfg, cls = gw.config("base", lnp.FIXTURE_LAYERS), WavLMForCTC
        cfg.vocab_size, cfg.pad_token_id, cfg.ctc_loss_reduction, cfg.ctc_zero_infinity = V, 0, "sum", False
        hw, hb = head_weights(iw, dims["n_state"], V)
        sd["lm_head.weight"], sd["lm_head.bias"] = torch.from_numpy(hw), torch.from_numpy(hb)
        models = {}
        for dt in (torch.float32, torch.float64):
            m = cls(cfg)
            m.load_state_dict(sd, strict=True)
            models[dt] = m.to(dt).eval()
        return models, hw, hb

    out, frames, inside_total = {}, 0, 0
    for model in ("xlsr", "wavlm"):
        models, hw, hb = build(model)
        V = VOCAB[model]
        for i in CLIPS:
            clip = wnp.make_clip(i, iw.uniform)
            key = f"{model}.clip{i}"
            with torch.no_grad():
                x64 = torch.from_numpy(clip)[None].double()
                o = models[torch.float64](x64, output_hidden_states=True)
                logits = o.logits[0]
                lp64 = logits.log_softmax(-1)
                lp32 = models[torch.float32](x64.float()).logits[0].log_softmax(-1).double()
                hidden = o.hidden_states[-1][0].numpy()
            T = lp64.shape[0]
            assert T == wnp.FRAMES[i], (T, wnp.FRAMES[i])
            am = float(lp64.abs().max())
            ids = logits.argmax(-1).numpy()
            # the head's own a-priori bound on the logits, from the model's last hidden state
            z = logits.numpy()
            assert np.abs(hidden @ hw.astype(np.float64).T + hb.astype(np.float64) - z).max() < 1e-9
            inside = cn.top2_gap(z) < 2 * cn.delta_z(hidden, hw, hb).max(axis=1)
            frames, inside_total = frames + T, inside_total + int(inside.sum())
            out[f"{key}.logprobs"] = lp64.numpy().astype(np.float32)
            out[f"{key}.ids"] = ids.astype(np.int64)
            out[f"{key}.greedy"] = cn.collapse(ids, 0)[0]
            out[f"{key}.inside"] = inside
            out[f"{key}.gap"] = np.float64(float((lp32 - lp64).abs().max()) / am)
            out[f"{key}.absmax"] = np.float64(am)
            print(f"{key}: {T} frames, log-probs absmax {am:.3f}, fp32 gap {out[f'{key}.gap']:.2e}, frames inside the gap {int(inside.sum())}, "
                  f"greedy tokens {len(out[f'{key}.greedy'])}")
            for L in LABEL_LENGTHS:
                lab = labels_of(iw, model, i, L, V)
                with torch.no_grad():
                    hf_labels = torch.from_numpy(lab)[None] if L else torch.full((1, 1), -100, dtype=torch.int64)
                    hf = float(models[torch.float64](x64, labels=hf_labels).loss)
                    loss = float(torch.nn.functional.ctc_loss(lp64[:, None], torch.from_numpy(lab)[None], torch.tensor([T]), torch.tensor([L]), blank=0,
                                                              reduction="sum", zero_infinity=False))
                mine, A = cn.forward(cn.emissions(lp64.numpy(), lab, 0), lab)
                if np.isfinite(loss):
                    assert abs(mine - loss) < 1e-9 * max(1.0, abs(loss)), (key, L, mine, loss)
                    assert abs(hf - loss) <= cn.bound3(T, A) + T * cn.U * am, (key, L, hf, loss)
                else:
                    assert mine == np.inf and hf == np.inf, (key, L, mine, hf)
                out[f"{key}.labels{L}"] = lab
                out[f"{key}.loss{L}"] = np.float64(loss)
                out[f"{key}.hfloss{L}"] = np.float64(hf)
                print(f"   L = {L}: loss {loss:.9g} (the model's own, on fp32 log-probs: {hf:.9g})")
    print(f"frames inside the gap: {inside_total} of {frames}")
    assert inside_total <= 0.01 * frames, (inside_total, frames)
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
