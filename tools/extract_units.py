"""Encode 16 kHz clips to Whisper units (the reference's 10_preprocess_train_unit.py flow; the counterpart of tools/extract_latents.py).

    python tools/extract_units.py IN [--out DIR] [--checkpoint pretrain/large-v3_encoder.pt | --synthetic [--layers N] [--seed S]] [--batch 8]

IN is a directory (every .npy / .wav in it, sorted) or a text file listing one clip per line.  A .npy holds 1-D float32 samples at
16 kHz; a .wav must be 16 kHz PCM16 (mono, or the first channel is taken) -- resampling is not built.  Every clip becomes
DIR/<name>.npy (default DIR: IN's directory + /units) of shape [T, n_audio_state], T = (len // 160 - 1) // 2 + 1.  Clips are batched
in sorted order through Units_Encoder.encode_ragged with their own lengths, so every clip's units are those of the clip encoded alone,
whatever its batch; clips shorter than 400 samples are zero-padded to 400 as Units_Encoder.encode does; clips over 30 s (more than
n_audio_ctx frames) are refused, as the data set's own preparation cuts them (00_del_audio_over_30s.py).
--synthetic runs seeded weights at large-v3's width (no checkpoint needed; --layers sets the depth, default 32).
"""
import argparse
import os
import sys
import wave

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "latent-diffusion-speech_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from encoder.whisper.model import ModelDimensions  # noqa: E402
from lds import arch  # noqa: E402
from tools.tools import Units_Encoder, WhisperLargeV3  # noqa: E402


def load_clip(path):
    if path.endswith(".npy"):
        return np.load(path).astype(np.float32).reshape(-1)
    with wave.open(path, "rb") as w:
        if w.getframerate() != 16000 or w.getsampwidth() != 2:
            raise ValueError(f"{path}: {w.getframerate()} Hz, {8 * w.getsampwidth()} bit; 16 kHz PCM16 is needed (resampling is not built)")
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype=np.int16).reshape(-1, w.getnchannels())[:, 0]
    return pcm.astype(np.float32) / 32768.0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("inp", help="directory of .npy / .wav clips, or a text file listing them")
    ap.add_argument("--out", default=None)
    ap.add_argument("--checkpoint", default="pretrain/large-v3_encoder.pt")
    ap.add_argument("--synthetic", action="store_true", help="seeded weights instead of the checkpoint")
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    if os.path.isdir(a.inp):
        base = a.inp
        paths = [os.path.join(a.inp, f) for f in sorted(os.listdir(a.inp)) if f.endswith((".npy", ".wav"))]
    else:
        base = os.path.dirname(os.path.abspath(a.inp))
        paths = [ln.strip() for ln in open(a.inp) if ln.strip()]
    out = a.out or os.path.join(base, "units")
    os.makedirs(out, exist_ok=True)
    if a.synthetic:
        model = WhisperLargeV3.synthetic(ModelDimensions(**dict(arch.WHISPER_LARGE_V3_DIMS, n_audio_layer=a.layers)), seed=a.seed, device="cuda")
    else:
        model = WhisperLargeV3(device="cuda", checkpoint=a.checkpoint)
    ue = Units_Encoder("whisper_large_v3", device="cuda", model=model)
    batch = max(1, min(a.batch, 64))
    for i in range(0, len(paths), batch):
        group = paths[i:i + batch]
        clips = [load_clip(p) for p in group]
        lens = [max(len(c), 400) for c in clips]
        audio = np.zeros((len(clips), max(lens)), dtype=np.float32)
        for b, c in enumerate(clips):
            audio[b, :len(c)] = c
        units, n_frames = ue.encode_ragged(torch.from_numpy(audio).cuda(), lens)
        units = units.cpu().numpy()
        for b, p in enumerate(group):
            np.save(os.path.join(out, os.path.splitext(os.path.basename(p))[0] + ".npy"), units[b, :int(n_frames[b])])
        print(f"{i + len(group)} / {len(paths)}")


if __name__ == "__main__":
    main()
