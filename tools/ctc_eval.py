"""Transcribe, score and align clips with a CTC head on a native speech encoder (encoder.ctc.CTCHead over Units_Encoder.encode_ragged).

    python tools/ctc_eval.py {transcribe,score,align} IN_DIR [--out DIR] [--checkpoint CTC.pt | --synthetic [--layers N] [--vocab V] [--seed S]]
                             [--encoder {xlsr_53_56k,wavlmbase+,wavlmlarge,contentvec768l12}] [--batch 8] [--sample-rate R]

IN_DIR holds clips: .npy samples at --sample-rate (default 16000) or PCM16 .wav of any rate, as tools/extract_units.py reads them; what is
not at 16 kHz is resampled on the device inside its batch.  Clips are batched in sorted order as ragged batches; a clip's result does not
depend on its batch.  --checkpoint: a local transformers *ForCTC state dict (torch-saved or .safetensors; config.json / vocab.json next
to it are read when present): its `lm_head` is the head, the rest (prefix stripped) the encoder.  --synthetic: seeded encoder and head.

  transcribe   DIR/NAME.json: the greedy transcript -- ids ("tokens"), "text" when the checkpoint has a vocab.json, and per token its first
               frame, run length, seconds and mean log-prob
  score        needs IN_DIR/NAME.labels.npy (int ids) per clip; DIR/scores.json: per clip nll = -log p(labels | clip), nll / L, and the
               character error rate of the greedy transcript against the labels (plain edit distance / L, on the host), and their means
  align        needs the same labels; DIR/NAME.align.json: the Viterbi path's log-probability and, per label, its segment in seconds
               (a frame is 320 samples at 16 kHz = 20 ms) and mean log-prob; "segments": null when the labels do not fit the clip
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

FRAME_SECONDS = 320 / 16000
ENCODERS = ("xlsr_53_56k", "wavlmbase+", "wavlmlarge", "contentvec768l12")


def build(a):
    """-> (Units_Encoder, CTCHead)"""
    from encoder.ctc import CTCHead, load_ctc_encoder_state
    from lds import arch
    from tools.tools import Audio2xlsr_53_56k, HubertUnits, Units_Encoder, WavLMUnits
    if a.synthetic:
        if a.encoder == "xlsr_53_56k":
            model = Audio2xlsr_53_56k.synthetic(dict(arch.XLSR_53_DIMS, n_layer=a.layers or 24), seed=a.seed, device="cuda")
        elif a.encoder == "contentvec768l12":
            model = HubertUnits.synthetic(a.encoder, dict(arch.HUBERT_BASE_DIMS, n_layer=a.layers or 12), seed=a.seed, device="cuda")
        else:
            dims = arch.wavlm_dims("large" if a.encoder == "wavlmlarge" else "base+")
            model = WavLMUnits.synthetic(a.encoder, dict(dims, n_layer=a.layers or dims["n_layer"]), seed=a.seed, device="cuda")
        head = CTCHead.synthetic(model.hidden_dim, a.vocab, seed=a.seed)
    else:
        if a.checkpoint is None:
            raise SystemExit("ctc_eval needs --checkpoint (a local transformers *ForCTC state dict) or --synthetic")
        head = CTCHead.from_checkpoint(a.checkpoint)
        with tempfile.TemporaryDirectory() as tmp:      # the existing loaders read a file: hand them the encoder half under its own names
            enc = os.path.join(tmp, "encoder.pt")
            torch.save(load_ctc_encoder_state(a.checkpoint), enc)
            if a.encoder == "xlsr_53_56k":
                model = Audio2xlsr_53_56k(device="cuda", checkpoint=enc)
            elif a.encoder == "contentvec768l12":
                model = HubertUnits(a.encoder, device="cuda", checkpoint=enc)
            else:
                model = WavLMUnits(a.encoder, device="cuda", checkpoint=enc)
    CTCHead.check_source(model)
    return Units_Encoder(a.encoder, device="cuda", model=model), head


def clip_paths(in_dir):
    return [os.path.join(in_dir, f) for f in sorted(os.listdir(in_dir)) if f.endswith((".npy", ".wav")) and not f.endswith(".labels.npy")]


def stem(path):
    return os.path.splitext(os.path.basename(path))[0]


def labels_of(path):
    lab = os.path.join(os.path.dirname(path), stem(path) + ".labels.npy")
    if not os.path.exists(lab):
        raise SystemExit(f"{lab} is missing: score and align need every clip's labels")
    return np.load(lab).astype(np.int64).reshape(-1)


def main(argv=None):
    from encoder.ctc import edit_distance
    from extract_units import encoder_batch, load_clip
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("command", choices=("transcribe", "score", "align"))
    ap.add_argument("in_dir")
    ap.add_argument("--out", default=None)
    ap.add_argument("--encoder", default="xlsr_53_56k", choices=ENCODERS)
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--synthetic", action="store_true", help="seeded encoder and head instead of a checkpoint")
    ap.add_argument("--layers", type=int, default=None, help="depth of the --synthetic encoder")
    ap.add_argument("--vocab", type=int, default=32, help="vocabulary of the --synthetic head")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--sample-rate", type=int, default=16000, help="rate of the .npy clips (a .wav carries its own)")
    a = ap.parse_args(argv)
    paths = clip_paths(a.in_dir)
    if not paths:
        raise SystemExit(f"no .npy / .wav clips in {a.in_dir}")
    out = a.out or os.path.join(os.path.dirname(os.path.abspath(a.in_dir)), "ctc_" + a.command)
    os.makedirs(out, exist_ok=True)
    ue, head = build(a)
    batch = max(1, min(a.batch, 64))
    scores = {}
    for i in range(0, len(paths), batch):
        group = paths[i:i + batch]
        audio, lens = encoder_batch([load_clip(p, a.sample_rate) for p in group], ue.min_samples)
        units, n_frames = ue.encode_ragged(audio, lens)
        n_frames = [int(n) for n in n_frames]
        greedy = head.greedy(units, n_frames) if a.command != "align" else None
        labels = [labels_of(p) for p in group] if a.command != "transcribe" else None
        if a.command == "transcribe":
            for p, g, n in zip(group, greedy, n_frames):
                rec = {"n_frames": n, "tokens": g["tokens"].tolist(), "text": head.decode(g["tokens"]) if head.vocab else None,
                       "start": g["start"].tolist(), "length": g["length"].tolist(),
                       "start_s": (g["start"] * FRAME_SECONDS).tolist(), "end_s": ((g["start"] + g["length"]) * FRAME_SECONDS).tolist(),
                       "logprob": [float(v) for v in g["logprob"]]}
                json.dump(rec, open(os.path.join(out, stem(p) + ".json"), "w"))
        elif a.command == "score":
            nll = head.score(units, n_frames, labels).cpu().numpy()
            for p, g, lab, v in zip(group, greedy, labels, nll):
                L = len(lab)
                fin = bool(np.isfinite(v))      # (labels that do not fit the clip: null, not a non-JSON Infinity)
                scores[stem(p)] = {"L": L, "nll": float(v) if fin else None, "nll_per_label": float(v) / max(L, 1) if fin else None,
                                   "cer": edit_distance(g["tokens"].tolist(), lab.tolist()) / max(L, 1)}
        else:
            for p, al, lab in zip(group, head.align(units, n_frames, labels), labels):
                ok = np.isfinite(al["score"])
                rec = {"score": al["score"] if ok else None,
                       "segments": [{"label": int(l), "start_s": float(s0 * FRAME_SECONDS), "end_s": float(s1 * FRAME_SECONDS), "logprob": float(lp)}
                                    for l, (s0, s1), lp in zip(lab, al["segments"], al["logprob"])] if ok else None}
                json.dump(rec, open(os.path.join(out, stem(p) + ".align.json"), "w"))
        print(f"{i + len(group)} / {len(paths)}")
    if a.command == "score":
        fin = [s for s in scores.values() if s["nll"] is not None]
        mean = {k: float(np.mean([s[k] for s in fin])) if fin else None for k in ("nll", "nll_per_label")}
        mean["cer"] = float(np.mean([s["cer"] for s in scores.values()]))
        json.dump({"clips": scores, "mean": mean}, open(os.path.join(out, "scores.json"), "w"), indent=1)
    print(f"{len(paths)} clips -> {out}")
    return out


if __name__ == "__main__":
    main()
