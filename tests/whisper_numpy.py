"""numpy restatement of the Whisper units encoder (reference encoder/whisper/audio.py:62-82, encoder/whisper/model.py:35-131,
tools/tools.py:118-126), in float32 or float64.  tests/test_cpu_units.py pins it to the fixtures recorded from the reference; the GPU
tests then use it at sizes the fixtures cannot hold (full width, 1500 frames)."""
import numpy as np
from scipy.special import erf

N_FFT, HOP = 400, 160


def frames_of(n_samples):
    """(mel frames, encoder frames) of a clip"""
    F = n_samples // HOP
    return F, (F - 1) // 2 + 1


def _basis(dtype):
    """windowed cos / sin basis [400][201] (periodic Hann), evaluated in float64 and rounded once to `dtype`"""
    i = np.arange(N_FFT, dtype=np.float64)
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * i / N_FFT)
    ang = 2.0 * np.pi * ((np.arange(N_FFT)[:, None] * np.arange(N_FFT // 2 + 1)[None, :]) % N_FFT) / N_FFT
    return (win[:, None] * np.cos(ang)).astype(dtype), (win[:, None] * np.sin(ang)).astype(dtype)


def log_mel(audio, filters, dtype=np.float32):
    """audio [n] (n >= 400) -> [n_mels][n // 160]: reflect padding, framed DFT as a product with the windowed basis, power, mel filter
    bank, log10, the clip's dynamic-range floor, (. + 4) / 4 -- every operation in `dtype`"""
    x = np.asarray(audio, dtype=dtype)
    n = x.shape[0]
    F = n // HOP
    xp = np.pad(x, (N_FFT // 2, N_FFT // 2), mode="reflect")
    fr = np.stack([xp[f * HOP:f * HOP + N_FFT] for f in range(F)])      # [F][400]
    bc, bs = _basis(dtype)
    re, im = fr @ bc, fr @ bs
    power = re * re + im * im                                              # [F][201]
    mel = np.asarray(filters, dtype=dtype) @ power.T
    lg = np.log10(np.maximum(mel, dtype(1e-10)))
    lg = np.maximum(lg, lg.max() - dtype(8.0))
    return ((lg + dtype(4.0)) / dtype(4.0)).astype(dtype)


def sinusoids(length, channels, dtype=np.float32):
    """model.py:35-40.  float32: the reference's operation order (the increment rounded to fp32 where torch multiplies the integer range
    by it, fp32 products) with exp / sin / cos of the fp32 arguments correctly rounded (evaluated in double, rounded once): an fp32 exp
    one ulp off moves the table by 1e-4 at frame 1500, and fp32 exp implementations differ by that, so the native table and this one
    are pinned to the definition every platform reproduces.  float64: the same lines in double"""
    inc = np.log(10000.0) / (channels // 2 - 1)
    if dtype == np.float32:
        arg = np.float32(-inc) * np.arange(channels // 2, dtype=np.float32)
        inv = np.exp(arg.astype(np.float64)).astype(np.float32)
        st = (np.arange(length, dtype=np.float32)[:, None] * inv[None, :]).astype(np.float64)
    else:
        inv = np.exp(-inc * np.arange(channels // 2, dtype=np.float64))
        st = np.arange(length, dtype=np.float64)[:, None] * inv[None, :]
    return np.concatenate([np.sin(st), np.cos(st)], axis=1).astype(dtype)


def _gelu(x):
    return (x * 0.5 * (1.0 + erf(x / np.sqrt(2.0)))).astype(x.dtype)


def _layer_norm(x, g, b, eps=1e-5):
    mu = x.mean(axis=-1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=-1, keepdims=True)
    return ((x - mu) / np.sqrt(var + x.dtype.type(eps)) * g + b).astype(x.dtype)


def _conv1d_k3(x, w, b, stride):
    """x [Ci][T], w [Co][Ci][3], padding 1 -> [Co][(T - 1) // stride + 1]"""
    T = x.shape[1]
    xp = np.pad(x, ((0, 0), (1, 1)))
    To = (T - 1) // stride + 1
    cols = np.stack([xp[:, k:k + stride * (To - 1) + 1:stride] for k in range(3)], axis=1)      # [Ci][3][To]
    return (w.reshape(w.shape[0], -1) @ cols.reshape(-1, To) + b[:, None]).astype(x.dtype)


def encoder(w, mel, n_head, dtype=np.float32):
    """AudioEncoder.forward for one clip: w = state_dict arrays ('encoder.*'), mel [n_mels][F] -> [T][n_state]"""
    W = {k: np.asarray(v, dtype=dtype) for k, v in w.items()}
    x = _gelu(_conv1d_k3(np.asarray(mel, dtype=dtype), W["encoder.conv1.weight"], W["encoder.conv1.bias"], 1))
    x = _gelu(_conv1d_k3(x, W["encoder.conv2.weight"], W["encoder.conv2.bias"], 2))
    x = x.T.copy()
    T, C = x.shape
    x = (x + sinusoids(T, C, dtype)).astype(dtype)
    D = C // n_head
    scale = dtype(D) ** dtype(-0.25)
    i = 0
    while f"encoder.blocks.{i}.attn_ln.weight" in W:
        p = f"encoder.blocks.{i}."
        h = _layer_norm(x, W[p + "attn_ln.weight"], W[p + "attn_ln.bias"])
        q = (h @ W[p + "attn.query.weight"].T + W[p + "attn.query.bias"]).reshape(T, n_head, D).transpose(1, 0, 2) * scale
        k = (h @ W[p + "attn.key.weight"].T).reshape(T, n_head, D).transpose(1, 2, 0) * scale
        v = (h @ W[p + "attn.value.weight"].T + W[p + "attn.value.bias"]).reshape(T, n_head, D).transpose(1, 0, 2)
        qk = (q @ k).astype(dtype)
        qk = qk - qk.max(axis=-1, keepdims=True)
        pr = np.exp(qk)
        pr = (pr / pr.sum(axis=-1, keepdims=True)).astype(dtype)
        a = (pr @ v).transpose(1, 0, 2).reshape(T, C)
        x = (x + a @ W[p + "attn.out.weight"].T + W[p + "attn.out.bias"]).astype(dtype)
        h = _layer_norm(x, W[p + "mlp_ln.weight"], W[p + "mlp_ln.bias"])
        h = _gelu((h @ W[p + "mlp.0.weight"].T + W[p + "mlp.0.bias"]).astype(dtype))
        x = (x + h @ W[p + "mlp.2.weight"].T + W[p + "mlp.2.bias"]).astype(dtype)
        i += 1
    return _layer_norm(x, W["encoder.ln_post.weight"], W["encoder.ln_post.bias"])


def encode(w, audio, filters, n_head, dtype=np.float32):
    """WhisperLargeV3.__call__ for one clip: audio [n] -> units [T][n_state]"""
    return encoder(w, log_mel(audio, filters, dtype), n_head, dtype)


def make_signal(name, n, seed, uniform, quiet_second_half=False):
    """the fixtures' kind of signal: a decaying sine plus white noise whose level switches between 0.1 and 0.002 three times a second,
    O(0.5) in amplitude; `uniform` = lds.init_weights.uniform"""
    t = np.arange(n, dtype=np.float64) / 16000.0
    noise = uniform(f"fix.{name}.noise", (n,), seed, -1.0, 1.0).astype(np.float64)
    gate = 0.02 + 0.98 * (np.sin(2.0 * np.pi * 3.0 * t) > 0).astype(np.float64)
    x = 0.5 * np.exp(-2.0 * t) * np.sin(2.0 * np.pi * 440.0 * t) + 0.1 * gate * noise
    if quiet_second_half:
        x[n // 2:] *= 1e-3
    return x.astype(np.float32)
