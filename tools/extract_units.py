"""Encode clips to units with Whisper large-v3 (default) or a HuBERT encoder (the reference's 10_preprocess_train_unit.py flow; the counterpart of tools/extract_latents.py).

    python tools/extract_units.py IN [--out DIR] [--checkpoint pretrain/large-v3_encoder.pt | --synthetic [--layers N] [--seed S]] [--batch 8]
                                     [--sample-rate R] [--encoder {whisper_large_v3,hubertsoft,contentvec768l12,xlsr_53_56k,w2v-bert,wavlmbase+,wavlmlarge}] [--units_layer N]

IN is a directory (every .npy / .wav in it, sorted) or a text file listing one clip per line.  A .npy holds 1-D float32 samples at
--sample-rate (default 16000); a .wav is PCM16 of any rate, read from its header (mono, or the first channel is taken).  Clips that
are not at 16 kHz are resampled on the device inside their batch (tools.tools.Resample.forward_ragged: every clip as if alone, the
reference's torchaudio Resample(rate, 16000)).  Every clip becomes DIR/<name>.npy (default DIR: IN's directory + /units) of shape
[T, n_audio_state], T = (len // 160 - 1) // 2 + 1 with len the clip's samples at 16 kHz.  Clips are batched in sorted order through
Units_Encoder.encode_ragged with their own lengths, so every clip's units are those of the clip encoded alone, whatever its batch;
clips shorter than 400 samples at 16 kHz are zero-padded to 400 as Units_Encoder.encode does; clips over 30 s (more than
n_audio_ctx frames, counted at 16 kHz) are refused, as the data set's own preparation cuts them (00_del_audio_over_30s.py).
--synthetic runs seeded weights at large-v3's width (no checkpoint needed; --layers sets the depth, default 32).
--encoder hubertsoft / contentvec768l12 runs the HuBERT stack instead (tools.tools.HubertUnits): [T, 256] / [T, 768], T = len // 320, clips
shorter than 320 samples zero-padded to 320; --checkpoint then names a HubertSoft state dict, and --synthetic's default depth is 12.
--encoder xlsr_53_56k runs wav2vec 2.0 XLSR-53 (tools.tools.Audio2xlsr_53_56k): [T, 1024], T by the unpadded level rule (400 samples -> 1
frame, 16000 -> 49); --checkpoint names a state dict of plain tensors in fairseq or transformers naming; --synthetic's default depth is 24.
--encoder w2v-bert runs w2v-BERT 2.0 (tools.tools.Wav2Vec2Bert): [rows, 1024], rows = ceil((1 + (len - 400) // 160) / 2) (16000 samples -> 49;
the last row of a clip with an odd frame count is the reference's masked row), clips shorter than 560 samples zero-padded to 560;
--checkpoint names the model's state dict in transformers naming (torch-saved or .safetensors); --synthetic's default depth is 24.
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
from tools.tools import Audio2xlsr_53_56k, HubertUnits, Resample, Units_Encoder, WavLMUnits, Wav2Vec2Bert, WhisperLargeV3  # noqa: E402

ENCODER_RATE = 16000
_resamplers = {}


def load_clip(path, npy_rate=ENCODER_RATE):
    """-> (samples float32 [L], their rate): a .npy at `npy_rate`, a PCM16 .wav at its header's rate"""
    if path.endswith(".npy"):
        return np.load(path).astype(np.float32).reshape(-1), int(npy_rate)
    with wave.open(path, "rb") as w:
        if w.getsampwidth() != 2:
            raise ValueError(f"{path}: {8 * w.getsampwidth()} bit; PCM16 is needed")
        rate = w.getframerate()
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype=np.int16).reshape(-1, w.getnchannels())[:, 0]
    return pcm.astype(np.float32) / 32768.0, rate


def encoder_batch(clips, min_samples=400):
    """[(samples, rate)] (at most 64) -> (audio [B, Lmax] on the device at 16 kHz, lengths [B]): the clips of every other rate go through
    one Resample.forward_ragged call per rate, each clip as if alone; a clip shorter than `min_samples` (400 for Whisper) counts as that
    many (zeros follow it)"""
    rows = [None] * len(clips)
    for rate in sorted({r for _, r in clips}):
        idx = [b for b, (_, r) in enumerate(clips) if r == rate]
        lens = [len(clips[b][0]) for b in idx]
        a = np.zeros((len(idx), max(lens)), dtype=np.float32)
        for k, b in enumerate(idx):
            a[k, :lens[k]] = clips[b][0]
        x = torch.from_numpy(a).cuda()
        if rate != ENCODER_RATE:
            if rate not in _resamplers:
                _resamplers[rate] = Resample(rate, ENCODER_RATE)
            x, lens = _resamplers[rate].forward_ragged(x, lens)
            lens = lens.tolist()
        for k, b in enumerate(idx):
            rows[b] = x[k, :lens[k]]
    lens = [max(int(r.numel()), min_samples) for r in rows]
    audio = torch.zeros((len(rows), max(lens)), dtype=torch.float32, device="cuda")
    for b, r in enumerate(rows):
        audio[b, :r.numel()] = r
    return audio, lens


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("inp", help="directory of .npy / .wav clips, or a text file listing them")
    ap.add_argument("--out", default=None)
    ap.add_argument("--encoder", default="whisper_large_v3", choices=("whisper_large_v3",) + HubertUnits.NAMES + ("xlsr_53_56k", "w2v-bert") + WavLMUnits.NAMES)
    ap.add_argument("--checkpoint", default=None, help="default: pretrain/large-v3_encoder.pt for whisper_large_v3; required for a HuBERT encoder")
    ap.add_argument("--synthetic", action="store_true", help="seeded weights instead of the checkpoint")
    ap.add_argument("--layers", type=int, default=None, help="depth of the --synthetic model (default 32; 12 for a HuBERT encoder, 24 for xlsr_53_56k, w2v-bert and wavlmlarge, 12 for wavlmbase+)")
    ap.add_argument("--units_layer", type=int, default=None, help="WavLM: the hidden state to store, 0 .. depth (default: the last layer; kNN-VC uses 6 of WavLM-Large)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--sample-rate", type=int, default=ENCODER_RATE, help="rate of the .npy clips (a .wav carries its own)")
    return ap


def main():
    ap = build_parser()
    a = ap.parse_args()
    if a.units_layer is not None and a.encoder not in WavLMUnits.NAMES:
        ap.error("--units_layer belongs to the WavLM encoders")
    if os.path.isdir(a.inp):
        base = a.inp
        paths = [os.path.join(a.inp, f) for f in sorted(os.listdir(a.inp)) if f.endswith((".npy", ".wav"))]
    else:
        base = os.path.dirname(os.path.abspath(a.inp))
        paths = [ln.strip() for ln in open(a.inp) if ln.strip()]
    out = a.out or os.path.join(base, "units")
    os.makedirs(out, exist_ok=True)
    if a.encoder in HubertUnits.NAMES:
        if a.synthetic:
            model = HubertUnits.synthetic(a.encoder, dict(arch.HUBERT_BASE_DIMS, n_layer=a.layers or 12), seed=a.seed, device="cuda")
        elif a.checkpoint is None:
            ap.error(f"--encoder {a.encoder} needs --checkpoint (a HubertSoft state dict) or --synthetic")
        else:
            model = HubertUnits(a.encoder, device="cuda", checkpoint=a.checkpoint)
    elif a.encoder == "xlsr_53_56k":
        if a.synthetic:
            model = Audio2xlsr_53_56k.synthetic(dict(arch.XLSR_53_DIMS, n_layer=a.layers or 24), seed=a.seed, device="cuda")
        elif a.checkpoint is None:
            ap.error("--encoder xlsr_53_56k needs --checkpoint (a wav2vec 2.0 state dict of plain tensors) or --synthetic")
        else:
            model = Audio2xlsr_53_56k(device="cuda", checkpoint=a.checkpoint)
    elif a.encoder == "w2v-bert":
        if a.synthetic:
            model = Wav2Vec2Bert.synthetic(dict(arch.W2V_BERT_DIMS, n_layer=a.layers or 24), seed=a.seed, device="cuda")
        elif a.checkpoint is None:
            ap.error("--encoder w2v-bert needs --checkpoint (the model's state dict in transformers naming) or --synthetic")
        else:
            model = Wav2Vec2Bert(device="cuda", checkpoint=a.checkpoint)
    elif a.encoder in WavLMUnits.NAMES:
        if a.synthetic:
            dims = arch.wavlm_dims("large" if a.encoder == "wavlmlarge" else "base+")
            model = WavLMUnits.synthetic(a.encoder, dict(dims, n_layer=a.layers or dims["n_layer"]), seed=a.seed, device="cuda", units_layer=a.units_layer)
        elif a.checkpoint is None:
            ap.error(f"--encoder {a.encoder} needs --checkpoint (the model's state dict in transformers naming) or --synthetic")
        else:
            model = WavLMUnits(a.encoder, device="cuda", checkpoint=a.checkpoint, units_layer=a.units_layer)
    elif a.synthetic:
        model = WhisperLargeV3.synthetic(ModelDimensions(**dict(arch.WHISPER_LARGE_V3_DIMS, n_audio_layer=a.layers or 32)), seed=a.seed, device="cuda")
    else:
        model = WhisperLargeV3(device="cuda", checkpoint=a.checkpoint or "pretrain/large-v3_encoder.pt")
    ue = Units_Encoder(a.encoder, device="cuda", model=model)
    batch = max(1, min(a.batch, 64))
    for i in range(0, len(paths), batch):
        group = paths[i:i + batch]
        audio, lens = encoder_batch([load_clip(p, a.sample_rate) for p in group], ue.min_samples)
        units, n_frames = ue.encode_ragged(audio, lens)
        units = units.cpu().numpy()
        for b, p in enumerate(group):
            np.save(os.path.join(out, os.path.splitext(os.path.basename(p))[0] + ".npy"), units[b, :int(n_frames[b])])
        print(f"{i + len(group)} / {len(paths)}")


if __name__ == "__main__":
    main()
