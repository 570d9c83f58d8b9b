"""Speaker embeddings and speaker similarity with an x-vector head on the native WavLM encoder (encoder.xvector.SpeakerEncoder).

    python tools/spk_eval.py embed CLIPS_DIR [--out DIR]   [--checkpoint XVECTOR.pt | --synthetic [--layers N] [--seed S]]
    python tools/spk_eval.py verify PAIRS.txt [--out FILE] [--encoder {wavlmbase+,wavlmlarge}] [--batch 8] [--sample-rate R]

Clips are .npy samples at --sample-rate (default 16000) or PCM16 .wav of any rate, as tools/extract_units.py reads them; what is not at
16 kHz goes through the native Resample on the device inside its batch.  Clips are batched in sorted order as ragged batches; a clip's
embedding does not depend on its batch.  A clip needs 5,200 samples at 16 kHz (16 encoder frames) with the default head geometry.
--checkpoint: a local transformers *ForXVector state dict (torch-saved or .safetensors; config.json next to it is read when present): its
projector / tdnn / feature_extractor / classifier (and layer_weights) are the head, the rest (prefix stripped) the encoder.  --synthetic:
seeded encoder and head.  Nothing is downloaded.

  embed    DIR/NAME.npy: the clip's embedding, float32 [xvector_dim]
  verify   PAIRS.txt holds one pair per line, `CLIP_A CLIP_B [LABEL]` (paths relative to the file; LABEL 1 = same speaker, 0 = not).  Prints
           the cosine per pair and, when every line has a label, the equal error rate; FILE (default PAIRS.txt + ".json") gets both.
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "latent-diffusion-speech_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

ENCODERS = ("wavlmbase+", "wavlmlarge")


def build(a):
    """-> SpeakerEncoder"""
    from encoder.xvector import SpeakerEncoder, XVectorHead, load_xvector_encoder_state
    from lds import arch
    from tools.tools import WavLMUnits
    if a.synthetic:
        dims = arch.wavlm_dims("large" if a.encoder == "wavlmlarge" else "base+")
        dims = dict(dims, n_layer=a.layers or dims["n_layer"])
        model = WavLMUnits.synthetic(a.encoder, dims, seed=a.seed, device="cuda")
        head = XVectorHead.synthetic(model.hidden_dim, seed=a.seed, n_layer=dims["n_layer"])
    else:
        if a.checkpoint is None:
            raise SystemExit("spk_eval needs --checkpoint (a local transformers *ForXVector state dict) or --synthetic")
        head = XVectorHead.from_checkpoint(a.checkpoint)
        with tempfile.TemporaryDirectory() as tmp:      # the existing loader reads a file: hand it the encoder half under its own names
            enc = os.path.join(tmp, "encoder.pt")
            torch.save(load_xvector_encoder_state(a.checkpoint), enc)
            model = WavLMUnits(a.encoder, device="cuda", checkpoint=enc)
    return SpeakerEncoder(model, head)


def embed_clips(spk, paths, a):
    """-> {path: embedding float32 [xvector_dim] on the host}"""
    from extract_units import encoder_batch, load_clip
    batch, out = max(1, min(a.batch, 64)), {}
    for i in range(0, len(paths), batch):
        group = paths[i:i + batch]
        audio, lens = encoder_batch([load_clip(p, a.sample_rate) for p in group], 400)
        emb = spk.embed_audio(audio, lens).cpu().numpy()
        out.update({p: e for p, e in zip(group, emb)})
    return out


def read_pairs(path):
    """-> [(clip a, clip b, label or None)] with absolute paths"""
    here, pairs = os.path.dirname(os.path.abspath(path)), []
    for n, line in enumerate(open(path), 1):
        f = line.split()
        if not f:
            continue
        if len(f) not in (2, 3) or (len(f) == 3 and f[2] not in ("0", "1")):
            raise SystemExit(f"{path}:{n}: expected `CLIP_A CLIP_B [0|1]`, got {line.strip()!r}")
        pairs.append((os.path.normpath(os.path.join(here, f[0])), os.path.normpath(os.path.join(here, f[1])), int(f[2]) if len(f) == 3 else None))
    if not pairs:
        raise SystemExit(f"no pairs in {path}")
    return pairs


def main(argv=None):
    from encoder.xvector import SpeakerEncoder, equal_error_rate
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("command", choices=("embed", "verify"))
    ap.add_argument("inp", help="embed: a directory of clips; verify: a text file of pairs")
    ap.add_argument("--out", default=None)
    ap.add_argument("--encoder", default="wavlmbase+", choices=ENCODERS)
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--synthetic", action="store_true", help="seeded encoder and head instead of a checkpoint")
    ap.add_argument("--layers", type=int, default=None, help="depth of the --synthetic encoder")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--sample-rate", type=int, default=16000, help="rate of the .npy clips (a .wav carries its own)")
    a = ap.parse_args(argv)
    if a.command == "embed":
        paths = [os.path.join(a.inp, f) for f in sorted(os.listdir(a.inp)) if f.endswith((".npy", ".wav"))]
        if not paths:
            raise SystemExit(f"no .npy / .wav clips in {a.inp}")
        out = a.out or os.path.join(os.path.dirname(os.path.abspath(a.inp)), "spk_embed")
        os.makedirs(out, exist_ok=True)
        for p, e in embed_clips(build(a), paths, a).items():
            np.save(os.path.join(out, os.path.splitext(os.path.basename(p))[0] + ".npy"), e.astype(np.float32))
        print(f"{len(paths)} clips -> {out}")
        return out
    pairs = read_pairs(a.inp)
    clips = sorted({p for pr in pairs for p in pr[:2]})
    emb = embed_clips(build(a), clips, a)
    table = torch.from_numpy(np.stack([emb[p] for p in clips])).cuda()
    sim = SpeakerEncoder.similarity(table, table).cpu().numpy()
    at = {p: i for i, p in enumerate(clips)}
    rows = []
    for pa, pb, lab in pairs:
        rows.append({"a": pa, "b": pb, "label": lab, "cosine": float(sim[at[pa], at[pb]])})
        print(f"{rows[-1]['cosine']:+.6f}  {pa}  {pb}" + ("" if lab is None else f"  {lab}"))
    eer = None
    if all(r["label"] is not None for r in rows):
        eer = equal_error_rate([r["cosine"] for r in rows], [r["label"] for r in rows])
        print(f"EER {100 * eer:.2f} % over {len(rows)} pairs")
    out = a.out or a.inp + ".json"
    json.dump({"pairs": rows, "eer": eer}, open(out, "w"), indent=1)
    return out


if __name__ == "__main__":
    main()
