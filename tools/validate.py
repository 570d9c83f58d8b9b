"""The validation pass of a units-to-mel checkpoint (the reference's diffusion/solver.py:9-85 `test`, without TensorBoard and audio files):
for every item (units, ground-truth latent, speaker id) it samples a mel, vocodes the sample and the ground truth, evaluates the diffusion
loss -- forward(infer=False) under no_grad -- and takes the log-mel spectrogram of both waveforms (vocoder.vocoder.get_mel).

    python tools/validate.py --model exp/diffusion/model_100000.pt --data VALID_DIR --out val.json [--method unipc] [--speedup 10] [--k_step N] [--dump DIR]
    python tools/validate.py --synthetic --items 2 --frames 24 --method unipc --speedup 250 --out val.json

VALID_DIR holds one <name>.npz per item with `units` [T, C] (the units encoder's output at the latent's frame rate), `latent` [T, M] (the
vocoder's latent of the ground-truth audio, Vocoder.extract) and `spk_id` (an integer).  --synthetic runs seeded weights on seeded items
instead (no checkpoint ships).  With --k_step the sample starts from q_sample(latent, k_step - 1), the shallow-diffusion entry, and the
loss draws its timesteps below k_step.  The JSON holds, per item and as means, the loss and the L1 distance between the two log-mels;
--dump DIR also writes <name>.pred_mel.npy / <name>.gt_mel.npy ([F, 128]).  --seed seeds torch's generator (the sampler's start noise and the
loss's timestep and noise draws)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "latent-diffusion-speech_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lds import native  # noqa: E402


def synthetic(n_items, frames, dev):
    from diffusion.unit2mel import Unit2Mel
    from diffusion.vocoder import Vocoder
    from encoder.hifi_vaegan.hifi_vaegan import Hifi_VAEGAN
    from lds import arch, init_weights
    h = arch.SYNTHETIC_VOCODER_H
    voc = Vocoder.__new__(Vocoder)
    voc.vocoder = Hifi_VAEGAN(None, device=dev, h=h, state=init_weights.init_state(arch.generator_param_shapes(h), 0))
    voc.vocoder_hop_size, voc.vocoder_sample_rate, voc.dimension, voc.device = h["hop_size"], h["sampling_rate"], h["inter_channels"], dev
    model = Unit2Mel(1280, 323, h["inter_channels"]).to(dev).eval()
    items = [(f"synthetic_{i}", init_weights.uniform(f"validate.units.{i}", (frames, 1280), 5, -1.7, 1.7),
              init_weights.uniform(f"validate.latent.{i}", (frames, h["inter_channels"]), 5, -0.9, 0.9), 1 + 7 * i) for i in range(n_items)]
    return model, voc, items


def load_items(path):
    for f in sorted(os.listdir(path)):
        if f.endswith(".npz"):
            z = np.load(os.path.join(path, f))
            yield f[:-4], z["units"].astype(np.float32), z["latent"].astype(np.float32), int(z["spk_id"])


@torch.no_grad()
def validate(model, vocoder, items, method="unipc", speedup=10, k_step=None, dump=None):
    """-> {"items": [{"name", "frames", "loss", "mel_l1"}], "loss", "mel_l1"}; the per-item steps in the reference's order"""
    dev = next(model.parameters()).device
    rows = []
    for name, units, latent, spk in items:
        units, latent = torch.from_numpy(units)[None].to(dev), torch.from_numpy(latent)[None].to(dev)
        spk_id = torch.tensor([[spk]], dtype=torch.int64, device=dev)
        if k_step is None:
            mel = model(units, None, spk_id, gt_spec=latent, infer=True, infer_speedup=speedup, method=method)
            loss = model(units, None, spk_id, gt_spec=latent, infer=False)
        else:      # Unit2Mel.forward has no k_step (reference unit2mel.py:73): the decoder is called on the embedded condition
            cond = native.transpose(model._native_embed().forward(units.contiguous(), spk_id))
            mel = model.decoder(cond, gt_spec=latent, infer=True, infer_speedup=speedup, method=method, k_step=k_step)
            loss = model.decoder(cond, gt_spec=latent, infer=False, k_step=k_step)
        signal = vocoder.infer(mel)
        gt_wav = vocoder.infer(latent)
        gt_mel = vocoder.vocoder.get_mel(gt_wav[0, ...])
        pred_mel = vocoder.vocoder.get_mel(signal[0, ...])
        dist = native.loss_reduce(pred_mel, gt_mel, "l1")
        rows.append({"name": name, "frames": int(pred_mel.shape[1]), "loss": float(loss), "mel_l1": float(dist)})
        if dump:
            np.save(os.path.join(dump, name + ".pred_mel.npy"), pred_mel[0].cpu().numpy())
            np.save(os.path.join(dump, name + ".gt_mel.npy"), gt_mel[0].cpu().numpy())
    if not rows:
        raise ValueError("no items to validate")
    return {"items": rows, "loss": float(np.mean([r["loss"] for r in rows])), "mel_l1": float(np.mean([r["mel_l1"] for r in rows]))}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", help="checkpoint model_<step>.pt with its config.yaml beside it (diffusion.unit2mel.load_model_vocoder)")
    ap.add_argument("--data", help="directory of <name>.npz items")
    ap.add_argument("--synthetic", action="store_true", help="seeded weights and items instead of --model / --data")
    ap.add_argument("--items", type=int, default=2, help="--synthetic: how many items")
    ap.add_argument("--frames", type=int, default=64, help="--synthetic: frames per item")
    ap.add_argument("--method", default="unipc")
    ap.add_argument("--speedup", type=int, default=10)
    ap.add_argument("--k_step", type=int, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", required=True, help="the JSON to write")
    ap.add_argument("--dump", default=None, help="directory for the log-mels as .npy")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/validate.py needs a HIP device (no CPU fallback)")
    dev = "cuda"
    if a.synthetic:
        model, vocoder, items = synthetic(a.items, a.frames, dev)
    else:
        if not a.model or not a.data:
            ap.error("--model and --data, or --synthetic")
        from diffusion.unit2mel import load_model_vocoder
        model, vocoder, _ = load_model_vocoder(a.model, device=dev)
        items = load_items(a.data)
    if a.dump:
        os.makedirs(a.dump, exist_ok=True)
    torch.manual_seed(a.seed)
    res = validate(model, vocoder, items, a.method, a.speedup, a.k_step, a.dump)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"items": len(res["items"]), "loss": res["loss"], "mel_l1": res["mel_l1"]}))


if __name__ == "__main__":
    main()
