"""Generate the HuBERT units encoder's golden fixtures by running the reference's own code.

Runs ONLY in the build container (needs /root/reference); the GPU box never sees the reference.  Writes (default: next to this
script, `--out DIR` elsewhere):

  hubert.npz             the reference's HubertSoft (encoder/hubert/model.py) with seeded weights (lds/arch.py hubert_init_state(
                         HUBERT_BASE_DIMS, seed 0), loaded with strict=True: that proves the keys) on five clips (tests/hubert_numpy.py
                         CLIPS: 320, 1,279, 41,277, 61,760 and 112,077 samples; regenerated from seeds by make_clip, never stored).
                         Per clip i: `rows_<i>` = the recorded frames (hubert_numpy.fixture_rows: all of a short clip, else the edges, the
                         tile boundaries and an even spread -- whole outputs of the long clips would exceed the repository's file size
                         limit) and, evaluated in float64 and stored rounded to float32, the rows of
                             feat_<i>   feature_extractor(pad(wav)) transposed          [rows][512]
                             l0_<i>, l2_<i>, l12_<i>   encode(pad(wav), layer=0 / 2 / None)[0]   [rows][768]
                             units_<i>  HubertSoft.units(wav)                           [rows][256]
                         (l12 / units for the three shorter clips only), each with `gap_<name>_<i>` = max |reference fp32 - reference fp64|
                         / absmax over the WHOLE output, and `absmax_<name>_<i>`.
  manifest_hubert.json   HubertSoft().state_dict() / HubertDiscrete(None).state_dict() key -> shape and str(inspect.signature(.)) of the
                         reference's public callables

The generator prints every stage's abs-max; all must lie in 0.1 .. 100 (asserted).

Import hygiene as in make_whisper_fixtures.py: the product directory is never on sys.path, only /root/reference is; arch.py,
init_weights.py and tests/hubert_numpy.py (for the clips and the row selection) are loaded by file path; an import-only placeholder stands
in for sklearn.cluster when the container lacks it (the reference imports KMeans for HubertDiscrete's codebook, which is not run here).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_hubert_fixtures.py [--out DIR]
    python tests/golden/make_hubert_fixtures.py --check      # regenerate into a temporary directory, compare bit for bit
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
FILES = ("manifest_hubert.json", "hubert.npz")
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
        print("hubert fixtures", "differ: " + ", ".join(bad) if bad else "reproduce bit for bit")
        return 1 if bad else 0


def main(out):
    arch = _load_by_path("_amd_arch", os.path.join(PKG, "lds", "arch.py"))
    init_weights = _load_by_path("_amd_init_weights", os.path.join(PKG, "lds", "init_weights.py"))
    hnp = _load_by_path("_amd_hubert_numpy", os.path.join(ROOT, "tests", "hubert_numpy.py"))
    sys.path[:] = [p for p in sys.path if os.path.realpath(p or ".") not in (os.path.realpath(PKG), os.path.realpath(ROOT), os.path.realpath(HERE))]
    sys.path.insert(0, REF)
    import torch
    import torch.nn.functional as F
    torch.set_grad_enabled(False)
    torch.set_num_threads(8)
    try:
        import sklearn.cluster  # noqa: F401
    except ImportError:
        _sk = _placeholder("sklearn.cluster", KMeans=object)
        _placeholder("sklearn", cluster=_sk)
    from encoder.hubert import model as ref
    f = os.path.realpath(ref.__file__)
    assert f.startswith(REF + os.sep), f"{ref} was imported from {f}, not from the reference"

    def tt(a):
        return torch.from_numpy(np.ascontiguousarray(a))

    # ---- manifest ----
    soft = ref.HubertSoft().eval()
    with torch.device("meta"):
        disc = ref.HubertDiscrete(None)
    sig = {
        "Hubert.__init__": str(inspect.signature(ref.Hubert.__init__)),
        "Hubert.encode": str(inspect.signature(ref.Hubert.encode)),
        "Hubert.forward": str(inspect.signature(ref.Hubert.forward)),
        "Hubert.logits": str(inspect.signature(ref.Hubert.logits)),
        "Hubert.mask": str(inspect.signature(ref.Hubert.mask)),
        "HubertSoft.__init__": str(inspect.signature(ref.HubertSoft.__init__)),
        "HubertSoft.units": str(inspect.signature(ref.HubertSoft.units)),
        "HubertDiscrete.__init__": str(inspect.signature(ref.HubertDiscrete.__init__)),
        "HubertDiscrete.units": str(inspect.signature(ref.HubertDiscrete.units)),
        "hubert_soft": str(inspect.signature(ref.hubert_soft)),
        "hubert_discrete": str(inspect.signature(ref.hubert_discrete)),
    }
    json.dump({"base_dims": arch.HUBERT_BASE_DIMS, "soft": {k: list(v.shape) for k, v in soft.state_dict().items()},
               "discrete": {k: list(v.shape) for k, v in disc.state_dict().items()}, "signatures": sig},
              open(os.path.join(out, "manifest_hubert.json"), "w"), indent=0)

    # ---- outputs ----
    state = arch.hubert_init_state(arch.HUBERT_BASE_DIMS, hnp.FIXTURE_SEED, init_weights)
    soft.load_state_dict({k: tt(v) for k, v in state.items()}, strict=True)
    soft64 = ref.HubertSoft().eval()
    soft64.load_state_dict({k: tt(v) for k, v in state.items()}, strict=True)
    soft64 = soft64.double()
    res = {}

    def stages(m, wav, full):
        x = F.pad(wav, (hnp.PAD, hnp.PAD))
        o = {"feat": m.feature_extractor(x).transpose(1, 2)[0], "l0": m.encode(x, layer=0)[0][0], "l2": m.encode(x, layer=2)[0][0]}
        if full:
            o["l12"] = m.encode(x)[0][0]
            o["units"] = m.units(wav)[0]
        return {k: v.numpy() for k, v in o.items()}

    for i, (n, seed) in enumerate(hnp.CLIPS):
        wav = tt(hnp.make_clip(i, init_weights.uniform)).view(1, 1, -1)
        full = i in hnp.FULL_DEPTH_CLIPS
        o32 = stages(soft, wav, full)
        o64 = stages(soft64, wav.double(), full)
        T = hnp.frames_of(n)
        rows = hnp.fixture_rows(T, hnp.MAX_ROWS[i])
        res[f"rows_{i}"] = rows
        for k in o64:
            assert o64[k].shape[0] == T == n // 320, (k, o64[k].shape, T)
            am = float(np.abs(o64[k]).max())
            assert 0.1 <= am <= 100.0, f"clip {i} stage {k}: abs-max {am} outside 0.1 .. 100"
            res[f"{k}_{i}"] = o64[k][rows].astype(np.float32)
            res[f"gap_{k}_{i}"] = np.float64(np.abs(o32[k].astype(np.float64) - o64[k]).max() / am)
            res[f"absmax_{k}_{i}"] = np.float64(am)
            print(f"clip {i} ({n} samples, {T} frames, {len(rows)} rows) {k}: absmax {am:.3f} rms {float(np.sqrt((o64[k] ** 2).mean())):.3f} "
                  f"fp32-vs-fp64 gap {res[f'gap_{k}_{i}']:.2e}")
    np.savez_compressed(os.path.join(out, "hubert.npz"), **res)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    if a.check:
        sys.exit(check())
    main(a.out)
