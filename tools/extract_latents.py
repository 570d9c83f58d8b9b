"""Encode a directory of float32 .npy waveforms to VAE latents (the reference's batch_proccessor/acoustic_extract.py flow).

    python tools/extract_latents.py IN_DIR OUT_DIR --model pretrain/hifi-vaegan [--batch 16] [--only-mean] [--ragged] [--sample-rate R]

Every IN_DIR/<name>.npy (1-D float32 at the vocoder's sample rate, or at --sample-rate: then every batch is resampled on the device
first, each clip as if alone, by tools.tools.Resample.forward_ragged -- the reference's torchaudio Resample(R, vocoder rate) -- and
len below is the resampled length) becomes OUT_DIR/<name>.npy of shape [ceil(len / hop), 2C] (m, then logs; zeros for logs with
--only-mean).  Files are batched in sorted order and right-padded with zeros to the longest clip of
their batch; each result is cropped to its own ceil(len / hop) frames afterwards.  That is the reference's own behaviour, and it means
that a clip's last frames can depend on its batch: the encoder's receptive field reaches into the padding of the batch, so a shorter clip
encoded with a longer one need not give what it gets alone.  With --ragged, each batch goes through Vocoder.extract_ragged with the clips'
own lengths instead, and every clip's latent is the clip encoded alone (within float rounding), independent of its batch.
"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "latent-diffusion-speech_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from diffusion.vocoder import Vocoder  # noqa: E402
from tools.tools import Resample  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("in_dir")
    ap.add_argument("out_dir")
    ap.add_argument("--model", required=True, help="directory with decoder.pth (config) and encoder.pth")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--only-mean", action="store_true", help="write zeros for logs (reference extract(only_mean=True))")
    ap.add_argument("--ragged", action="store_true", help="encode every clip as if alone (extract_ragged with the clips' own lengths)")
    ap.add_argument("--sample-rate", type=int, default=None, help="rate of the clips (default: the vocoder's)")
    a = ap.parse_args()
    voc = Vocoder("hifi-vaegan", a.model, device="cuda")
    hop = voc.vocoder_hop_size
    rs = None
    if a.sample_rate not in (None, voc.vocoder_sample_rate):
        rs = Resample(a.sample_rate, voc.vocoder_sample_rate)
        a.batch = min(a.batch, 64)      # (the ragged resampler's batch limit)
    names = sorted(f for f in os.listdir(a.in_dir) if f.endswith(".npy"))
    os.makedirs(a.out_dir, exist_ok=True)
    for i in range(0, len(names), a.batch):
        group = names[i:i + a.batch]
        clips = [np.load(os.path.join(a.in_dir, f)).astype(np.float32).reshape(-1) for f in group]
        L = max(len(c) for c in clips)
        audio = np.zeros((len(clips), L), dtype=np.float32)
        for b, c in enumerate(clips):
            audio[b, :len(c)] = c
        x, lens = torch.from_numpy(audio).cuda(), [len(c) for c in clips]
        if rs is not None:
            x, lens = rs.forward_ragged(x, lens)
            lens = lens.tolist()
        if a.ragged:
            lat = voc.extract_ragged(x, voc.vocoder_sample_rate, lens, only_mean=a.only_mean).cpu().numpy()
        else:
            lat = voc.extract(x, voc.vocoder_sample_rate, only_mean=a.only_mean).cpu().numpy()
        for b, f in enumerate(group):
            np.save(os.path.join(a.out_dir, f), lat[b, :math.ceil(lens[b] / hop)])
        print(f"{i + len(group)} / {len(names)}")


if __name__ == "__main__":
    main()
