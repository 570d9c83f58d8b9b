"""A recording in, the converted recording out: DiffusionSVC.infer_from_long_audio (reference tools/infer_tools.py:83-117) from the
command line.  The recording is cut at its silences, the segments go through the Whisper units encoder, the diffusion sampler and the
vocoder as ragged batches, and one kernel joins them under the volume mask.

    python infer_svc.py -dm exp/diffusion/model_300000.pt -ue pretrain/large-v3_encoder.pt -i in.wav -o out.wav
    python infer_svc.py --synthetic -i in.wav -o out.wav          # seeded random weights (no checkpoints exist)
    python infer_svc.py --synthetic -o out.wav                    # ... and a generated recording of --synthetic_seconds
    python infer_svc.py ... --index units_index.pt --index_ratio 0.5 --index_k 8      # units retrieval over the target speaker's pool
    python infer_svc.py ... --index units_index.pt --index_nprobe 8                   # ... through the file's IVF (train_units_index.py --nlist)
"""
import argparse
import os
import sys
import wave

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "latent-diffusion-speech_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("-dm", "--diffusion_model")
    ap.add_argument("-ue", "--units_encoder", help="large-v3_encoder.pt: {'dims', 'model_state_dict'} of the Whisper encoder")
    ap.add_argument("--encoder", default="whisper_large_v3", choices=("whisper_large_v3", "hubertsoft", "contentvec768l12", "xlsr_53_56k", "wavlmbase+", "wavlmlarge"),
                    help="the units encoder; for a HuBERT encoder -ue names a HubertSoft state dict, for xlsr_53_56k a wav2vec 2.0 state dict of "
                         "plain tensors (fairseq or transformers naming), for a WavLM encoder its state dict in transformers naming")
    ap.add_argument("-i", "--input", help="mono PCM16 .wav, or .npy float [L] (then --sample_rate says its rate)")
    ap.add_argument("-sr", "--sample_rate", type=int, default=44100, help="rate of a .npy input / of the generated recording")
    ap.add_argument("-o", "--output", default="output.wav", help=".wav (PCM16) or .npy")
    ap.add_argument("-id", "--spk_id", type=int, default=1)
    ap.add_argument("-s", "--speedup", type=int, default=10)
    ap.add_argument("-me", "--method", default="unipc")
    ap.add_argument("-th", "--threhold", type=float, default=-60.0, help="volume mask threshold, dB")
    ap.add_argument("--threhold_for_split", type=float, default=-40.0)
    ap.add_argument("--min_len", type=int, default=5000, help="shortest piece the slicer cuts, ms")
    ap.add_argument("--batch_size", type=int, default=16, help="segments per ragged batch (1 .. 64; 1 = the reference's loop shape)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--index", help="units_index.pt (tools/train_units_index.py): every units frame is blended with its nearest rows of this pool "
                                    "before the diffusion model (units retrieval, exact and on the device)")
    ap.add_argument("--index_ratio", type=float, default=0.5, help="0 .. 1: the share of the retrieved units in the blend")
    ap.add_argument("--index_k", type=int, default=8, help="1 .. 8 nearest pool rows per frame")
    ap.add_argument("--index_nprobe", type=int, default=None, help="1 .. 8: search only the rows of a frame's N best lists (an index written with --nlist)")
    ap.add_argument("--index_weights", default="inverse_square", choices=("inverse_square", "uniform"),
                    help="the blend's weights: 1 / d^2 over the distances, or the plain mean of the rows found (kNN-VC: --index_k 4 --index_ratio 1.0 "
                         "over an index written with --metric cosine; the metric comes from the index file)")
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--synthetic_width", type=int, default=1280, help="width of the synthetic units encoder (a multiple of 64)")
    ap.add_argument("--synthetic_layers", type=int, default=4)
    ap.add_argument("--synthetic_seconds", type=float, default=12.0)
    return ap.parse_args(argv)


def synthetic_svc(dev, width=1280, layers=4, encoder="whisper_large_v3", encoder_dims=None):
    """DiffusionSVC with seeded random-init weights throughout (no checkpoints ship with the reference): the Unit2Mel and
    vocoder of infer_tts.synthetic_pipeline, a Whisper encoder of `width` (large-v3's mel front end and context) with resampling on; or,
    for encoder 'hubertsoft' / 'contentvec768l12', the HuBERT-base stack of `layers` blocks (its own width: 256 / 768); or, for
    'xlsr_53_56k', the XLSR-53 network of `layers` blocks (1024 wide), or of `encoder_dims` (lds.arch.XLSR_53_DIMS' fields) when given; or,
    for 'wavlmbase+' / 'wavlmlarge', that WavLM of `layers` blocks (768 / 1024 wide), or of `encoder_dims` (lds_wavlm_cfg's fields)"""
    from diffusion.unit2mel import DotDict, Unit2Mel
    from diffusion.vocoder import Vocoder
    from encoder.hifi_vaegan.hifi_vaegan import Hifi_VAEGAN
    from encoder.whisper.model import ModelDimensions
    from lds import arch, init_weights
    from tools.infer_tools import DiffusionSVC
    from tools.tools import Audio2xlsr_53_56k, HubertUnits, Units_Encoder, Volume_Extractor, WavLMUnits, WhisperLargeV3
    h = arch.SYNTHETIC_VOCODER_H
    if encoder in HubertUnits.NAMES:
        width = arch.get_encoder_out_channels(encoder)
    if encoder == "xlsr_53_56k":
        encoder_dims = dict(arch.XLSR_53_DIMS, n_layer=layers) if encoder_dims is None else dict(encoder_dims)
        width = encoder_dims["n_state"]
    if encoder in WavLMUnits.NAMES:
        base = arch.wavlm_dims("large" if encoder == "wavlmlarge" else "base+")
        encoder_dims = dict(base, n_layer=layers) if encoder_dims is None else dict(encoder_dims)
        width = encoder_dims["n_state"]
    voc = Vocoder.__new__(Vocoder)
    voc.vocoder = Hifi_VAEGAN(None, device=dev, h=h, state=init_weights.init_state(arch.generator_param_shapes(h), 0))
    voc.vocoder_hop_size, voc.vocoder_sample_rate, voc.dimension, voc.device = h["hop_size"], h["sampling_rate"], h["inter_channels"], dev
    svc = DiffusionSVC(device=dev)
    svc.model, svc.vocoder = Unit2Mel(width, 323, h["inter_channels"]).to(dev).eval(), voc
    svc.args = DotDict({"data": {"block_size": h["hop_size"], "sampling_rate": h["sampling_rate"], "encoder": encoder,
                                 "encoder_sample_rate": 16000, "encoder_hop_size": 320}})
    if encoder in HubertUnits.NAMES:
        model = HubertUnits.synthetic(encoder, dict(arch.HUBERT_BASE_DIMS, n_layer=layers), seed=0, device=dev)
    elif encoder == "xlsr_53_56k":
        model = Audio2xlsr_53_56k.synthetic(encoder_dims, seed=0, device=dev)
    elif encoder in WavLMUnits.NAMES:
        model = WavLMUnits.synthetic(encoder, encoder_dims, seed=0, device=dev)
    else:
        dims = ModelDimensions(**dict(arch.WHISPER_LARGE_V3_DIMS, n_audio_state=width, n_audio_head=width // 64, n_audio_layer=layers))
        model = WhisperLargeV3.synthetic(dims, seed=0, device=dev)
    svc.units_encoder = Units_Encoder(encoder, 16000, 320, device=dev, model=model, resample=True)
    svc.volume_extractor = Volume_Extractor(hop_size=512, block_size=h["hop_size"], model_sampling_rate=h["sampling_rate"])
    return svc


def synthetic_recording(seconds, sr, seed=0):
    """phrases of a wandering tone, 0.4 .. 6 s long, separated by near-silences of 0.35 .. 1.2 s: what a slicer cuts into segments of
    mixed lengths.  fp32 [round(seconds * sr)]"""
    rng = np.random.default_rng(seed)
    n = int(round(seconds * sr))
    t = np.arange(n) / float(sr)
    env = np.full(n, 2e-4)
    pos, i = 0.2, 0
    while pos < seconds - 0.5:
        dur = (0.9, 0.4, 1.7, 3.0, 6.0)[i % 5] * rng.uniform(0.8, 1.2)
        i += 1
        a, b = int(pos * sr), min(int((pos + dur) * sr), n)
        env[a:b] = rng.uniform(0.15, 0.3) * np.minimum(1.0, np.minimum(np.arange(b - a), np.arange(b - a)[::-1]) / (0.02 * sr))
        pos += dur + rng.uniform(0.35, 1.2)
    phase = 2 * np.pi * np.cumsum(180.0 + 60.0 * np.sin(2 * np.pi * 0.7 * t)) / sr
    return (np.maximum(env, 2e-4) * np.sin(phase)).astype(np.float32)


def read_audio(path, sample_rate):
    if path.endswith(".npy"):
        return np.load(path).astype(np.float32).reshape(-1), sample_rate
    with wave.open(path, "rb") as f:
        if f.getsampwidth() != 2:
            raise SystemExit(f"{path}: only PCM16 .wav files are read")
        pcm = np.frombuffer(f.readframes(f.getnframes()), dtype="<i2").reshape(-1, f.getnchannels())
        return (pcm.astype(np.float32).mean(axis=1) / 32768.0).astype(np.float32), f.getframerate()


def main(argv=None):
    a = parse_args(argv)
    dev = "cuda"
    if a.synthetic:
        svc = synthetic_svc(dev, a.synthetic_width, a.synthetic_layers, a.encoder)
    else:
        if not a.diffusion_model or not a.units_encoder:
            raise SystemExit("-dm and -ue are needed (or --synthetic)")
        from tools.infer_tools import DiffusionSVC
        svc = DiffusionSVC(device=dev)
        svc.load_model(a.diffusion_model, units_encoder_checkpoint=a.units_encoder, resample=True,
                       encoder=None if a.encoder == "whisper_large_v3" else a.encoder)
    if a.input:
        audio, sr = read_audio(a.input, a.sample_rate)
    elif a.synthetic:
        audio, sr = synthetic_recording(a.synthetic_seconds, a.sample_rate), a.sample_rate
    else:
        raise SystemExit("-i is needed")
    index = None
    if a.index:
        from cluster.index import UnitsIndex
        index = UnitsIndex.load(a.index)
    torch.manual_seed(a.seed)
    wav, rate = svc.infer_from_long_audio(audio, sr=sr, spk_id=a.spk_id, infer_speedup=a.speedup, method=a.method, threhold=a.threhold,
                                          threhold_for_split=a.threhold_for_split, min_len=a.min_len, batch_size=a.batch_size, index=index,
                                          index_ratio=a.index_ratio, index_k=a.index_k, index_nprobe=a.index_nprobe, index_weights=a.index_weights)
    wav = wav.cpu().numpy()
    if a.output.endswith(".wav"):
        with wave.open(a.output, "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(rate)
            f.writeframes((np.clip(wav, -1, 1) * 32767).astype("<i2").tobytes())
    else:
        np.save(a.output, wav)
    print(f"wrote {a.output}: {wav.shape[0]} samples ({wav.shape[0] / rate:.2f} s at {rate} Hz) from {audio.shape[0]} samples at {sr} Hz")
    return wav


if __name__ == "__main__":
    main()
