"""Speech to text with Whisper: clips of any rate -> Resample -> the native audio encoder (encode_ragged) -> the native text decoder (greedy).

    python tools/transcribe.py CLIPS_DIR [--out DIR] [--synthetic [--layers N] [--seed S] | --checkpoint large-v3.pt] [--language en]
                                         [--task transcribe] [--max-new-tokens 224] [--batch 8] [--sample-rate R] [--tokenizer DIR]

CLIPS_DIR is a directory (every .npy / .wav in it, sorted) or a text file listing one clip per line, read as tools/extract_units.py reads
them.  --checkpoint names an official OpenAI file ({"dims", "model_state_dict"}: both halves load unchanged); --synthetic runs seeded
weights at large-v3's dimensions (--layers sets both depths, default 32) and exists to exercise the pipeline: its "transcripts" mean
nothing.  Every clip becomes DIR/<name>.tokens.npy (the generated ids, prompt and <|endoftext|> removed; default DIR: CLIPS_DIR +
/transcripts), and DIR/transcripts.json holds per clip the ids, `avg_logprob` (the mean log-prob of the generated ids, <|endoftext|>
included) and, with --tokenizer, the text.  --tokenizer must name a LOCAL directory that transformers' WhisperTokenizer can load
(vocab.json, merges.txt, ...): nothing is ever downloaded, a name that is not a directory is refused.  The special-token ids come from
lds.arch.whisper_special_tokens (unverified against a tokenizer file; with --tokenizer they are checked against it before anything runs).
Clips beyond 30 s are refused: long-form decoding (windows, timestamps, temperature fallback) is not built.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "latent-diffusion-speech_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

MAX_SECONDS = 30


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("inp", metavar="CLIPS_DIR", help="directory of .npy / .wav clips, or a text file listing them")
    ap.add_argument("--out", default=None)
    src = ap.add_mutually_exclusive_group()
    src.add_argument("--checkpoint", default=None, help="an OpenAI Whisper checkpoint: {'dims', 'model_state_dict'}")
    src.add_argument("--synthetic", action="store_true", help="seeded weights at large-v3's dimensions")
    ap.add_argument("--layers", type=int, default=None, help="depth of both halves of the --synthetic model (default 32)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--language", default="en")
    ap.add_argument("--task", default="transcribe", choices=("transcribe", "translate"))
    ap.add_argument("--max-new-tokens", type=int, default=224)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--sample-rate", type=int, default=16000, help="rate of the .npy clips (a .wav carries its own)")
    ap.add_argument("--tokenizer", default=None, help="a LOCAL directory with WhisperTokenizer's files; never a hub name")
    return ap


def check_args(ap, a):
    """what can be refused before any model is built"""
    if not a.synthetic and a.checkpoint is None:
        ap.error("give --checkpoint large-v3.pt or --synthetic")
    if a.tokenizer is not None and not os.path.isdir(a.tokenizer):
        ap.error(f"--tokenizer {a.tokenizer!r} is not a local directory: nothing is downloaded, a hub name is refused")
    if a.layers is not None and not a.synthetic:
        ap.error("--layers belongs to --synthetic")
    if not 1 <= a.batch <= 64:
        ap.error("--batch must be in 1 .. 64")
    if a.max_new_tokens < 1:
        ap.error("--max-new-tokens must be positive")
    return a


def load_tokenizer(path):
    from transformers import WhisperTokenizer
    return WhisperTokenizer.from_pretrained(path, local_files_only=True)


def main(argv=None):
    ap = build_parser()
    a = check_args(ap, ap.parse_args(argv))
    import numpy as np
    import torch
    from encoder.whisper.model import ModelDimensions, Whisper
    from extract_units import encoder_batch, load_clip
    from lds import arch
    if a.synthetic:
        n = a.layers or 32
        dims = ModelDimensions(**dict(arch.WHISPER_LARGE_V3_DIMS, n_audio_layer=n, n_text_layer=n))
        state = arch.whisper_init_state(dims.n_mels, dims.n_audio_state, dims.n_audio_layer, a.seed)
        state.update(arch.whisper_decoder_init_state(dims.n_vocab, dims.n_text_ctx, dims.n_text_state, dims.n_text_layer, a.seed))
    else:
        ck = torch.load(a.checkpoint, map_location="cpu", weights_only=False)
        dims, state = ModelDimensions(**ck["dims"]), ck["model_state_dict"]
    model = Whisper(dims, decoder=True)
    model.load_state_dict({k: torch.as_tensor(v).float() for k, v in state.items()})
    model.eval()
    sp = model.special_tokens()
    tok = load_tokenizer(a.tokenizer) if a.tokenizer else None
    if tok is not None:      # the derived table against the tokenizer that came with the checkpoint
        for name, text in (("eot", "<|endoftext|>"), ("sot", "<|startoftranscript|>"), ("transcribe", "<|transcribe|>"), ("translate", "<|translate|>"),
                           ("notimestamps", "<|notimestamps|>"), ("startofprev", "<|startofprev|>")):
            got = tok.convert_tokens_to_ids(text)
            if got != sp[name]:
                raise SystemExit(f"the tokenizer has {text} at {got}, the derived table at {sp[name]}: pass the ids to Whisper.decode yourself")
    if a.language not in sp["languages"]:
        ap.error(f"unknown --language {a.language!r}")
    if os.path.isdir(a.inp):
        base = a.inp
        paths = [os.path.join(a.inp, f) for f in sorted(os.listdir(a.inp)) if f.endswith((".npy", ".wav"))]
    else:
        base = os.path.dirname(os.path.abspath(a.inp))
        paths = [ln.strip() for ln in open(a.inp) if ln.strip()]
    out = a.out or os.path.join(base, "transcripts")
    os.makedirs(out, exist_ok=True)
    enc = model.encoder.native()
    report = {}
    for i in range(0, len(paths), a.batch):
        group = paths[i:i + a.batch]
        clips = [load_clip(p, a.sample_rate) for p in group]
        for p, (x, rate) in zip(group, clips):
            if len(x) > MAX_SECONDS * rate:
                raise SystemExit(f"{p}: {len(x) / rate:.1f} s; clips beyond {MAX_SECONDS} s are refused (long-form decoding is not built)")
        audio, lens = encoder_batch(clips, 400)
        ln = enc.lengths(lens, len(group), audio.shape[1])
        units = enc.encode(audio.float().contiguous(), ln)
        n_frames = [(int(v) // 160 - 1) // 2 + 1 for v in ln]
        # the prompt is built here, so that what is cut off a row below is the prompt that row was given
        prompts = [[sp["sot"], sp["languages"][a.language], sp[a.task], sp["notimestamps"]] for _ in group]
        toks, tlp, avg = model.decode(units, n_frames, prompt=prompts, max_new_tokens=a.max_new_tokens)
        toks, avg = toks.cpu().numpy(), avg.cpu().numpy()
        for b, p in enumerate(group):
            ids = [int(t) for t in toks[b, len(prompts[b]):]]
            ids = ids[: ids.index(sp["eot"])] if sp["eot"] in ids else ids
            name = os.path.splitext(os.path.basename(p))[0]
            np.save(os.path.join(out, name + ".tokens.npy"), np.asarray(ids, dtype=np.int64))
            report[name] = {"tokens": ids, "avg_logprob": float(avg[b])}
            if tok is not None:
                report[name]["text"] = tok.decode(ids, skip_special_tokens=True)
        print(f"{i + len(group)} / {len(paths)}")
    json.dump(report, open(os.path.join(out, "transcripts.json"), "w"), indent=1, ensure_ascii=False)


if __name__ == "__main__":
    main()
