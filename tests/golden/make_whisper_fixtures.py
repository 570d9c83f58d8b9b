"""Generate the Whisper units encoder's golden fixtures by running the reference's own code.

Runs ONLY in the build container (needs /root/reference); the GPU box never sees the reference.  Writes (default: next to this
script, `--out DIR` elsewhere):

  whisper_mel_filters.npz   the reference's two filter banks (encoder/whisper/assets/mel_filters.npz: data), mel_80 / mel_128
  whisper_logmel_128.npz, whisper_logmel_80.npz
                            log_mel_spectrogram (reference encoder/whisper/audio.py:62-82) of five clips: 400, 1,600, 48,000 and 112,077
                            samples (odd frame count, not a multiple of 160) and 64,000 samples with the second half scaled by 1e-3
                            (exercises the `max - 8` floor).  Per clip: `ref64_<i>` = the same lines evaluated in float64 (restated below
                            with torch in double), stored rounded to float32 (6e-8 on values of O(1): 0.2 % of E_ref; one file per n_mels
                            keeps every file below the repository's size limit), `eref_<i>` = max |reference fp32 - reference fp64| over
                            the whole array (from the unrounded float64 result), `n_<i>`, `seed_<i>`, `quiet_<i>`.  The audio is not
                            stored: tests/whisper_numpy.py make_signal regenerates it from the seed.
  whisper_encoder.npz       AudioEncoder.forward (reference encoder/whisper/model.py:112-131) on seeded weights (lds/arch.py
                            whisper_init_state, seed 0): (n_mels 128, n_state 128, 2 heads, 4 layers) on a mel of 400 frames and
                            (80, 256, 4, 3) on a mel of 37 frames (odd), mel = uniform in [-1, 1.5) from a seed; and the body of
                            WhisperLargeV3.__call__ (tools/tools.py:118-126: view(1, -1), log_mel_spectrogram, encoder, squeeze) for one clip
                            of 16,000 samples with the first configuration.  `gap_*` = max |fp32 - fp64| / absmax of the reference itself
                            (for the end-to-end case: fp32 mel into the fp32 stack against fp64 mel into the fp64 stack).
  manifest_whisper.json     Whisper(dims).state_dict() key -> shape for large-v3's dims and the small configuration, and
                            str(inspect.signature(.)) of the reference's Units_Encoder / WhisperLargeV3 / log_mel_spectrogram / mel_filters

One line of the reference cannot run here: model.py:40 ends `sinusoids` with `.to(device="cuda")`.  The recipe wraps torch.Tensor.to for
the duration of that call so that the `device` keyword is dropped; the values remain the reference's own arithmetic.  For the float64
evaluations only, the reference's LayerNorm subclass (model.py:23-25, which casts its input to float32) runs nn.LayerNorm.forward.

Import hygiene as in make_encoder_fixtures.py: the product directory is never on sys.path, only /root/reference is; arch.py,
init_weights.py and tests/whisper_numpy.py (for make_signal only) are loaded by file path; import-only placeholders stand in for the
packages tools/tools.py imports and the container lacks (librosa, fairseq, transformers, torchaudio).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_whisper_fixtures.py [--out DIR]
    python tests/golden/make_whisper_fixtures.py --check      # regenerate into a temporary directory, compare bit for bit
"""
import argparse
import importlib.util
import inspect
import json
import os
import subprocess
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PKG = os.path.join(ROOT, "latent-diffusion-speech_amd")
REF = "/root/reference"
FILES = ("manifest_whisper.json", "whisper_mel_filters.npz", "whisper_logmel_128.npz", "whisper_logmel_80.npz", "whisper_encoder.npz")
CLIPS = ((400, 31, False), (1600, 32, False), (48000, 33, False), (112077, 34, False), (64000, 35, True))      # (samples, seed, quiet second half)
SMALL = dict(n_mels=128, n_audio_ctx=1500, n_audio_state=128, n_audio_head=2, n_audio_layer=4, n_vocab=1, n_text_ctx=1, n_text_state=1,
             n_text_head=1, n_text_layer=1)
SMALL_B = dict(SMALL, n_mels=80, n_audio_state=256, n_audio_head=4, n_audio_layer=3)
sys.dont_write_bytecode = True


def _load_by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _placeholder(name, **attrs):
    import importlib.machinery
    m = types.ModuleType(name)
    m.__spec__ = importlib.machinery.ModuleSpec(name, None)
    for k, v in attrs.items():
        setattr(m, k, v)
    return sys.modules.setdefault(name, m)


def check():
    """regenerate into a temporary directory (PYTHONPATH-free child) and compare with the committed files bit for bit"""
    with tempfile.TemporaryDirectory() as out_dir:
        env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
        env.pop("PYTHONPATH", None)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--out", out_dir], env=env, cwd=out_dir,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            print(r.stdout[-4000:])
            return 1
        bad = []
        for f in FILES:
            a, b = os.path.join(HERE, f), os.path.join(out_dir, f)
            if f.endswith(".json"):
                if json.load(open(a)) != json.load(open(b)):
                    bad.append(f)
                continue
            za, zb = np.load(a), np.load(b)
            if sorted(za.files) != sorted(zb.files):
                bad.append(f)
                continue
            for k in za.files:
                x, y = za[k], zb[k]
                if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
                    bad.append(f"{f}:{k}")
        print("whisper fixtures", "differ: " + ", ".join(bad) if bad else "reproduce bit for bit")
        return 1 if bad else 0


def main(out):
    arch = _load_by_path("_amd_arch", os.path.join(PKG, "lds", "arch.py"))
    init_weights = _load_by_path("_amd_init_weights", os.path.join(PKG, "lds", "init_weights.py"))
    wnp = _load_by_path("_amd_whisper_numpy", os.path.join(ROOT, "tests", "whisper_numpy.py"))
    sys.path[:] = [p for p in sys.path if os.path.realpath(p or ".") not in (os.path.realpath(PKG), os.path.realpath(ROOT), os.path.realpath(HERE))]
    sys.path.insert(0, REF)
    import torch
    torch.set_grad_enabled(False)
    torch.set_num_threads(8)
    _placeholder("librosa")
    _placeholder("fairseq", checkpoint_utils=None)
    _placeholder("transformers", AutoFeatureExtractor=object, Wav2Vec2BertModel=object)
    _tat = _placeholder("torchaudio.transforms", Resample=object)
    _placeholder("torchaudio", transforms=_tat)
    from encoder.whisper import audio as ref_audio, model as ref_model
    from tools import tools as ref_tools
    for m in (ref_audio, ref_model, ref_tools):
        f = os.path.realpath(m.__file__)
        assert f.startswith(REF + os.sep), f"{m} was imported from {f}, not from the reference"

    # model.py:40 `.to(device="cuda")`: drop the device keyword while sinusoids runs, nothing else
    real_sinusoids = ref_model.sinusoids

    def cpu_sinusoids(*a, **k):
        real_to = torch.Tensor.to

        def to_no_device(self, *aa, **kk):
            kk.pop("device", None)
            return real_to(self, *aa, **kk) if (aa or kk) else self
        torch.Tensor.to = to_no_device
        try:
            return real_sinusoids(*a, **k)
        finally:
            torch.Tensor.to = real_to
    ref_model.sinusoids = cpu_sinusoids

    def tt(a):
        return torch.from_numpy(np.ascontiguousarray(a))

    # ---- manifest ----
    def shapes(dims):
        with torch.device("meta"):
            enc = ref_model.AudioEncoder(dims["n_mels"], dims["n_audio_state"], dims["n_audio_head"], dims["n_audio_layer"])
        return {"encoder." + k: list(v.shape) for k, v in enc.state_dict().items()}
    small_model = ref_model.Whisper(ref_model.ModelDimensions(**SMALL))
    assert list(small_model.state_dict().keys()) == list(shapes(SMALL).keys())      # Whisper(dims) holds the encoder only
    sig = {
        "Units_Encoder.__init__": str(inspect.signature(ref_tools.Units_Encoder.__init__)),
        "Units_Encoder.encode": str(inspect.signature(ref_tools.Units_Encoder.encode)),
        "WhisperLargeV3.__init__": str(inspect.signature(ref_tools.WhisperLargeV3.__init__)),
        "WhisperLargeV3.__call__": str(inspect.signature(ref_tools.WhisperLargeV3.__call__)),
        "log_mel_spectrogram": str(inspect.signature(ref_audio.log_mel_spectrogram)),
        "mel_filters": str(inspect.signature(ref_audio.mel_filters.__wrapped__)),
        "AudioEncoder.__init__": str(inspect.signature(ref_model.AudioEncoder.__init__)),
    }
    json.dump({"large_v3_dims": arch.WHISPER_LARGE_V3_DIMS, "large_v3": shapes(arch.WHISPER_LARGE_V3_DIMS), "small_dims": SMALL,
               "small": shapes(SMALL), "signatures": sig}, open(os.path.join(out, "manifest_whisper.json"), "w"), indent=0)

    # ---- filter banks (data) ----
    banks = {n: ref_audio.mel_filters("cpu", n).numpy().copy() for n in (80, 128)}
    np.savez_compressed(os.path.join(out, "whisper_mel_filters.npz"), mel_80=banks[80], mel_128=banks[128])

    # ---- log-mel ----
    def logmel64(audio, n_mels):
        """audio.py:72-82 in float64"""
        a = audio.double()
        window = torch.hann_window(ref_audio.N_FFT, dtype=torch.float64)
        stft = torch.stft(a, ref_audio.N_FFT, ref_audio.HOP_LENGTH, window=window, return_complex=True)
        magnitudes = stft[..., :-1].abs() ** 2
        mel_spec = ref_audio.mel_filters("cpu", n_mels).double() @ magnitudes
        log_spec = torch.clamp(mel_spec, min=1e-10).log10()
        log_spec = torch.maximum(log_spec, log_spec.max() - 8.0)
        return (log_spec + 4.0) / 4.0

    for n_mels in (128, 80):
        res = {}
        for i, (n, seed, quiet) in enumerate(CLIPS):
            audio = wnp.make_signal(f"clip{i}", n, seed, init_weights.uniform, quiet)
            r32 = ref_audio.log_mel_spectrogram(tt(audio), n_mels=n_mels).numpy()
            r64 = logmel64(tt(audio), n_mels).numpy()
            assert r32.shape == r64.shape == (n_mels, n // 160)
            res[f"ref64_{i}"] = r64.astype(np.float32)
            res[f"eref_{i}"] = np.float64(np.abs(r32.astype(np.float64) - r64).max())
            res[f"n_{i}"] = np.int64(n)
            res[f"seed_{i}"] = np.int64(seed)
            res[f"quiet_{i}"] = np.int64(quiet)
            print(f"logmel n_mels {n_mels} clip {i} ({n} samples): E_ref {res[f'eref_{i}']:.3e} absmax {np.abs(r64).max():.3f} "
                  f"at the floor {float((r64 <= r64.min() + 1e-12).mean()):.3f}")
        np.savez_compressed(os.path.join(out, f"whisper_logmel_{n_mels}.npz"), **res)

    # ---- encoder ----
    res = {}

    class in_double:
        """model.py:23-25 casts LayerNorm's input to float32: for a float64 evaluation run the parent's forward"""
        def __enter__(self):
            self.real = ref_model.LayerNorm.forward
            ref_model.LayerNorm.forward = torch.nn.LayerNorm.forward

        def __exit__(self, *a):
            ref_model.LayerNorm.forward = self.real

    def build(dims):
        model = ref_model.Whisper(ref_model.ModelDimensions(**dims))
        state = arch.whisper_init_state(dims["n_mels"], dims["n_audio_state"], dims["n_audio_layer"], 0, init_weights)
        model.load_state_dict({k: tt(v) for k, v in state.items()})
        return model.eval()

    for name, dims, F, seed in (("a", SMALL, 400, 41), ("b", SMALL_B, 37, 42)):
        model = build(dims)
        mel = init_weights.uniform(f"fix.whisper.{name}.mel", (1, dims["n_mels"], F), seed, -1.0, 1.5)
        o32 = model.encoder(tt(mel)).numpy()
        with in_double():
            o64 = model.double().encoder(tt(mel).double()).numpy()
        res[f"{name}_out"] = o32
        res[f"{name}_gap"] = np.float64(np.abs(o32 - o64).max() / np.abs(o64).max())
        res[f"{name}_dims"] = np.array([dims["n_mels"], dims["n_audio_state"], dims["n_audio_head"], dims["n_audio_layer"], F, seed], dtype=np.int64)
        print(f"encoder {name}: out {o32.shape} absmax {np.abs(o32).max():.3f} fp32-vs-fp64 gap {res[f'{name}_gap']:.2e}")
    # the body of WhisperLargeV3.__call__ (tools/tools.py:118-126) with the first configuration
    model = build(SMALL)
    audio = tt(wnp.make_signal("e2e", 16000, 43, init_weights.uniform, False))

    def call_body(model, audio, mel_fn):
        audio = audio.view(1, -1)
        mel = mel_fn(audio)
        if len(mel.shape) == 2:
            mel = mel.unsqueeze(0)
        return model.encoder(mel).squeeze().data.cpu()
    u32 = call_body(model, audio, ref_audio.log_mel_spectrogram).float().numpy()
    with in_double():
        u64 = call_body(model.double(), audio, lambda a: logmel64(a, 128)).numpy()
    res["e2e_out"] = u32
    res["e2e_gap"] = np.float64(np.abs(u32 - u64).max() / np.abs(u64).max())
    res["e2e_n"] = np.int64(16000)
    res["e2e_seed"] = np.int64(43)
    print(f"end to end: out {u32.shape} absmax {np.abs(u32).max():.3f} fp32-vs-fp64 gap {res['e2e_gap']:.2e}")
    np.savez_compressed(os.path.join(out, "whisper_encoder.npz"), **res)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    if a.check:
        sys.exit(check())
    main(a.out)
