"""Generate the VAE encoder's golden fixtures by running the reference's own `Hifi_VAEGAN.extract`.

Runs ONLY in the build container (needs /root/reference); the GPU box never sees the reference.  Writes (default: next to this
script, `--out DIR` elsewhere):

  manifest_encoder.json  Encoder.state_dict() key -> shape for arch.SYNTHETIC_VOCODER_H (reference encoder/hifi_vaegan/modules/models.py:14-37)
  encoder.npz            Hifi_VAEGAN.extract (reference hifi_vaegan.py:32-50) on seeded weights (lds/init_weights.py, seed 0), B = 2 and
                         L = 12 * 512 - 100 samples (extract pads to 12 frames): the default output [B,T,2C], only_mean, and
                         only_z + only_mean, with the randn_like draw of every call recorded
  encoder_rb2.npz        the same with resblock '2' (h2 as in make_fixtures.py)

The reference is driven through a temporary model directory holding torch.save'd decoder.pth (config) / encoder.pth (weights), so its
padding, only_z and only_mean lines are in the fixture rather than restated here.  torch.randn_like is replaced by a recording version
on a seeded CPU generator for each call.

Test audio: uniform in [-0.5, 0.5).  With the seeded weights (weight_g in [0.5, 1.5), so every output row of every convolution has a
norm of about one) the encoder keeps the signal at O(1) through all five stages: m and logs come out with absmax 0.3 - 0.45, so
exp(logs) neither overflows nor vanishes and z (absmax about 4) is a meaningful comparison; no rescaling was needed.

Import hygiene as in make_fixtures.py: the product directory is never on sys.path, only /root/reference is; arch.py and
init_weights.py are loaded by file path; import-only placeholders stand in for the packages the container lacks
(vector_quantize_pytorch, torchaudio, and librosa / soundfile, which the reference's nvSTFT imports but STFT.__init__ never calls).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_encoder_fixtures.py [--out DIR]
    python tests/golden/make_encoder_fixtures.py --check      # regenerate into a temporary directory, compare bit for bit
"""
import argparse
import importlib.util
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
FILES = ("manifest_encoder.json", "encoder.npz", "encoder_rb2.npz")
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
        print("encoder fixtures", "differ: " + ", ".join(bad) if bad else "reproduce bit for bit")
        return 1 if bad else 0


def main(out):
    arch = _load_by_path("_amd_arch", os.path.join(PKG, "lds", "arch.py"))
    init_weights = _load_by_path("_amd_init_weights", os.path.join(PKG, "lds", "init_weights.py"))
    sys.path[:] = [p for p in sys.path if os.path.realpath(p or ".") not in (os.path.realpath(PKG), os.path.realpath(ROOT), os.path.realpath(HERE))]
    sys.path.insert(0, REF)
    import torch
    torch.set_grad_enabled(False)
    torch.set_num_threads(8)
    _placeholder("vector_quantize_pytorch", VectorQuantize=object)
    _tat = _placeholder("torchaudio.transforms", Spectrogram=object, Resample=object, MelSpectrogram=object)
    _placeholder("torchaudio", transforms=_tat)
    _lf = _placeholder("librosa.filters", mel=None)
    _placeholder("librosa", filters=_lf)
    _placeholder("soundfile")
    from encoder.hifi_vaegan import hifi_vaegan as ref_hv
    from encoder.hifi_vaegan.modules.models import Encoder
    for obj in (ref_hv, Encoder):
        f = os.path.realpath(sys.modules[obj.__name__].__file__ if isinstance(obj, types.ModuleType) else sys.modules[obj.__module__].__file__)
        assert f.startswith(REF + os.sep), f"{obj} was imported from {f}, not from the reference"

    def tt(a):
        return torch.from_numpy(np.ascontiguousarray(a))

    h = arch.SYNTHETIC_VOCODER_H
    json.dump({k: list(v.shape) for k, v in Encoder(h).state_dict().items()}, open(os.path.join(out, "manifest_encoder.json"), "w"), indent=0)

    real_randn_like = torch.randn_like

    def run(hh, name, seed):
        state = {k: tt(v) for k, v in init_weights.init_state(arch.encoder_param_shapes(hh), 0).items()}
        B, L = 2, 12 * 512 - 100
        audio = init_weights.uniform(f"fix.{name}.audio", (B, L), seed, -0.5, 0.5)
        res = {"audio": audio, "h_json": np.frombuffer(json.dumps(hh, sort_keys=True).encode(), dtype=np.uint8)}
        with tempfile.TemporaryDirectory() as d:
            torch.save({"config": hh, "model": {}}, os.path.join(d, "decoder.pth"))
            torch.save({"model": state}, os.path.join(d, "encoder.pth"))
            vae = ref_hv.Hifi_VAEGAN(d, device="cpu")
            gen = torch.Generator().manual_seed(seed)
            draws = []

            def recording_randn_like(x, *a, **k):
                n = torch.randn(x.shape, generator=gen, dtype=x.dtype)
                draws.append(n.numpy().copy())
                return n

            torch.randn_like = recording_randn_like
            try:
                res["out"] = vae.extract(tt(audio)).numpy()
                res["noise"] = draws[-1]
                res["out_mean"] = vae.extract(tt(audio), only_mean=True).numpy()
                res["noise_mean"] = draws[-1]
                res["z_mean"] = vae.extract(tt(audio), only_z=True, only_mean=True).numpy()
                res["noise_z"] = draws[-1]
            finally:
                torch.randn_like = real_randn_like
        C = hh["inter_channels"]
        m, logs = res["out"][..., :C], res["out"][..., C:]
        print(name, res["out"].shape, "absmax m", float(np.abs(m).max()), "logs", float(np.abs(logs).max()), "z", float(np.abs(res["z_mean"]).max()))
        assert np.all(np.isfinite(res["z_mean"])) and np.abs(logs).max() < 20
        np.savez_compressed(os.path.join(out, f"{name}.npz"), **res)

    run(h, "encoder", 21)
    run(dict(h, resblock="2", resblock_dilation_sizes=[[1, 3], [1, 3], [1, 3]]), "encoder_rb2", 22)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    if a.check:
        sys.exit(check())
    main(a.out)
