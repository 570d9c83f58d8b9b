"""Turn unit files, or audio clips, into semantic tokens (the reference's 19_preprocess_token.py, its kmeans branch).

    python tools/extract_tokens.py IN_DIR [--out DIR] [--codebook pretrain/semantic_codebook.pt | --synthetic K [--seed S]] [--batch 8]
                                   [--from-audio [--checkpoint pretrain/large-v3_encoder.pt | --synthetic-encoder [--layers N]]
                                    [--sample-rate R] [--encoder {whisper_large_v3,hubertsoft,contentvec768l12,w2v-bert}]]

IN_DIR holds .npy unit files [T, dim] (tools/extract_units.py writes them).  Every file becomes DIR/<name>.npy (default DIR:
IN_DIR/../semantic_token) of int64 tokens [T]: the index of the nearest centre of the codebook, computed on the HIP device by
cluster.get_cluster_result.  Files are batched in sorted order, padded to the longest of the batch and assigned in the ragged form, so
a file's tokens do not depend on its batch.  --synthetic K uses K seeded N(0, 1) centres instead of a checkpoint.
--from-audio: IN_DIR holds clips instead (.npy samples at --sample-rate, default 16000, or PCM16 .wav of any rate, as
tools/extract_units.py reads them; what is not at 16 kHz is resampled on the device inside its batch); every batch goes through
Units_Encoder.encode_tokens_ragged (Whisper units, then the nearest centre) without leaving the device.  --synthetic-encoder
runs seeded encoder weights at large-v3's width (--layers sets the depth) where no checkpoint exists.  --encoder hubertsoft /
contentvec768l12 encodes with the HuBERT stack instead (tools.tools.HubertUnits; --checkpoint then names a HubertSoft state dict);
--encoder w2v-bert with w2v-BERT 2.0 (tools.tools.Wav2Vec2Bert; --checkpoint names its state dict in transformers naming).
"""
import argparse
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "latent-diffusion-speech_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import cluster  # noqa: E402


def units_encoder(a):
    from encoder.whisper.model import ModelDimensions
    from lds import arch
    from tools.tools import HubertUnits, Units_Encoder, Wav2Vec2Bert, WhisperLargeV3
    if a.encoder in HubertUnits.NAMES:
        if a.synthetic_encoder:
            model = HubertUnits.synthetic(a.encoder, dict(arch.HUBERT_BASE_DIMS, n_layer=a.layers or 12), seed=a.seed, device="cuda")
        elif a.checkpoint is None:
            raise SystemExit(f"--encoder {a.encoder} needs --checkpoint (a HubertSoft state dict) or --synthetic-encoder")
        else:
            model = HubertUnits(a.encoder, device="cuda", checkpoint=a.checkpoint)
    elif a.encoder == "w2v-bert":
        if a.synthetic_encoder:
            model = Wav2Vec2Bert.synthetic(dict(arch.W2V_BERT_DIMS, n_layer=a.layers or 24), seed=a.seed, device="cuda")
        elif a.checkpoint is None:
            raise SystemExit("--encoder w2v-bert needs --checkpoint (the model's state dict in transformers naming) or --synthetic-encoder")
        else:
            model = Wav2Vec2Bert(device="cuda", checkpoint=a.checkpoint)
    elif a.synthetic_encoder:
        model = WhisperLargeV3.synthetic(ModelDimensions(**dict(arch.WHISPER_LARGE_V3_DIMS, n_audio_layer=a.layers or 32)), seed=a.seed, device="cuda")
    else:
        model = WhisperLargeV3(device="cuda", checkpoint=a.checkpoint or "pretrain/large-v3_encoder.pt")
    return Units_Encoder(a.encoder, device="cuda", model=model)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("in_dir")
    ap.add_argument("--out", default=None)
    ap.add_argument("--codebook", default="pretrain/semantic_codebook.pt")
    ap.add_argument("--synthetic", type=int, default=0, metavar="K")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--metric", default="l2", choices=("l2", "cosine"), help="cosine: the centre of highest cosine similarity (a codebook from "
                    "train_codebook.py --mode cosine)")
    ap.add_argument("--from-audio", action="store_true", help="IN_DIR holds audio clips: encode them to units first")
    ap.add_argument("--sample-rate", type=int, default=16000, help="--from-audio: rate of the .npy clips (a .wav carries its own)")
    ap.add_argument("--encoder", default="whisper_large_v3", choices=("whisper_large_v3", "hubertsoft", "contentvec768l12", "w2v-bert"))
    ap.add_argument("--checkpoint", default=None, help="default: pretrain/large-v3_encoder.pt for whisper_large_v3")
    ap.add_argument("--synthetic-encoder", action="store_true", help="seeded encoder weights instead of the checkpoint")
    ap.add_argument("--layers", type=int, default=None, help="depth of the synthetic encoder (default 32; 12 for a HuBERT encoder)")
    a = ap.parse_args()
    ext = (".npy", ".wav") if a.from_audio else (".npy",)
    paths = [os.path.join(a.in_dir, f) for f in sorted(os.listdir(a.in_dir)) if f.endswith(ext)]
    if not paths:
        raise SystemExit(f"no {' / '.join(ext)} files in {a.in_dir}")
    out = a.out or os.path.join(os.path.dirname(os.path.abspath(a.in_dir)), "semantic_token")
    os.makedirs(out, exist_ok=True)
    ue = units_encoder(a) if a.from_audio else None
    if a.synthetic:
        dim = getattr(ue.model.hidden_dim, "n_audio_state", ue.model.hidden_dim) if a.from_audio else np.load(paths[0]).shape[1]
        model = types.SimpleNamespace(cluster_centers_=np.random.default_rng(a.seed).standard_normal((a.synthetic, dim)).astype(np.float32))
    else:
        model = cluster.get_cluster_model(a.codebook)
    batch = max(1, min(a.batch, 64))
    for i in range(0, len(paths), batch):
        group = paths[i: i + batch]
        if a.from_audio:
            from extract_units import encoder_batch, load_clip      # (tools/ is this script's own directory)
            audio, slen = encoder_batch([load_clip(p, a.sample_rate) for p in group], ue.min_samples)      # (16 kHz on the device; at least the encoder's shortest clip each)
            tok, lens = ue.encode_tokens_ragged(audio, slen, model, pad_id=-1, metric=a.metric)
            tok, lens = tok.cpu().numpy(), [int(n) for n in lens]
        else:
            units = [np.load(p).astype(np.float32) for p in group]
            lens = [u.shape[0] for u in units]
            x = np.zeros((len(units), max(lens), units[0].shape[1]), dtype=np.float32)
            for b, u in enumerate(units):
                x[b, : lens[b]] = u
            tok = cluster.get_cluster_result(model, torch.from_numpy(x).cuda(), lengths=lens, pad_id=-1, metric=a.metric).cpu().numpy()
        for b, p in enumerate(group):
            np.save(os.path.join(out, os.path.splitext(os.path.basename(p))[0] + ".npy"), tok[b, : lens[b]])
    print(f"{len(paths)} files -> {out}")


if __name__ == "__main__":
    main()
