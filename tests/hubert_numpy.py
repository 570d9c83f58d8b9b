"""numpy restatement of the HuBERT units encoder (reference encoder/hubert/model.py:19-148) for any lds_hubert_cfg, in float32 or
float64: what the CPU suite holds against the reference's fixtures and the GPU suite against the library where no fixture exists
(reduced configurations).  One clip at a time, as the reference runs."""
import numpy as np
from scipy.special import erf

PAD = 40
FIXTURE_SEED = 0
# (samples, seed) of the fixture clips: 1 frame; floors that drop frames; the positional kernel's width; a whole 128-tap window inside;
# a frame count that is a multiple of neither 4 nor 32
CLIPS = ((320, 51), (1279, 52), (41277, 53), (61760, 54), (112077, 55))
FULL_DEPTH_CLIPS = (0, 1, 2)      # the clips whose 12-layer outputs are recorded
MAX_ROWS = (1, 3, 20, 24, 32)     # recorded rows per clip (the files must stay below the repository's size limit)


def frames_of(n_samples, pad=PAD):
    n = (int(n_samples) + 2 * pad - 10) // 5 + 1
    for i in range(1, 7):
        n = (n - 3) // 2 + 1 if i <= 4 else (n - 2) // 2 + 1
    return n


def level_frames(n_samples, pad=PAD):
    """frames after conv0 .. conv6"""
    out = [(int(n_samples) + 2 * pad - 10) // 5 + 1]
    for i in range(1, 7):
        out.append((out[-1] - 3) // 2 + 1 if i <= 4 else (out[-1] - 2) // 2 + 1)
    return out


def fixture_rows(T, n):
    """The frames of a T-frame output that the fixtures record: all of them when T <= n, else the edges, the neighbours of the 32- / 64- /
    128-frame tile boundaries and an even spread, n in all."""
    if T <= n:
        return np.arange(T, dtype=np.int64)
    want = [0, 1, T - 2, T - 1, 31, 32, 63, 64, 127, 128, 191, 192, 255, 256]
    rows = []
    for r in want:
        if 0 <= r < T and r not in rows and len(rows) < n:
            rows.append(r)
    for r in np.linspace(2, T - 3, 4 * n).astype(np.int64):
        if len(rows) >= n:
            break
        if int(r) not in rows:
            rows.append(int(r))
    return np.array(sorted(rows), dtype=np.int64)


def make_clip(i, uniform):
    """fixture clip i: uniform noise in [-1, 1) under a slow envelope (regenerated from the seed, never stored)"""
    n, seed = CLIPS[i]
    x = uniform(f"fix.hubert.clip{i}", (n,), seed, -1.0, 1.0)
    env = (0.55 + 0.45 * np.sin(np.arange(n, dtype=np.float64) * (2.0 * np.pi / 4001.0))).astype(np.float32)
    return (x * env).astype(np.float32)


def _mm(a, b):
    """a @ b with the products summed in float64 and the result rounded to the operands' type: in float32 this is the library's
    "exact fp32" contract (fp32 tensors between operators) without an accumulation order of its own"""
    return (np.asarray(a, dtype=np.float64) @ np.asarray(b, dtype=np.float64)).astype(a.dtype)


def _gelu(x):
    return (x * 0.5 * (1.0 + erf(x / np.sqrt(2.0)))).astype(x.dtype)


def _layer_norm(x, g, b, eps=1e-5):
    """over the last axis"""
    x64 = x.astype(np.float64)
    mu = x64.mean(axis=-1, keepdims=True)
    var = ((x64 - mu) ** 2).mean(axis=-1, keepdims=True)
    return (((x64 - mu) / np.sqrt(var + eps)).astype(x.dtype) * g + b).astype(x.dtype)


def _conv1d(x, w, stride):
    """x [Ci][T], w [Co][Ci][K], no padding, no bias -> [Co][To]"""
    Co, Ci, K = w.shape
    To = (x.shape[1] - K) // stride + 1
    cols = np.concatenate([np.ascontiguousarray(x[:, k:k + stride * (To - 1) + 1:stride]) for k in range(K)], axis=0)      # [K Ci][To]
    return _mm(np.ascontiguousarray(w.transpose(0, 2, 1)).reshape(Co, K * Ci), cols)


def fold_weight_norm(g, v):
    v64 = np.asarray(v, dtype=np.float64)
    n = np.sqrt((v64 * v64).sum(axis=(0, 1), keepdims=True))
    return np.asarray(g, dtype=np.float64).reshape(1, 1, -1) * v64 / n


def features(w, audio, dtype=np.float32, pad=PAD):
    """FeatureExtractor.forward on the clip padded by `pad` zeros per side -> [T][conv_dim]"""
    W = lambda k: np.asarray(w[k], dtype=dtype)
    x = np.concatenate([np.zeros(pad, dtype), np.asarray(audio, dtype=dtype), np.zeros(pad, dtype)])[None, :]
    y = _conv1d(x, W("feature_extractor.conv0.weight"), 5)
    y = _layer_norm(y, 1.0, 0.0).astype(dtype) * W("feature_extractor.norm0.weight")[:, None] + W("feature_extractor.norm0.bias")[:, None]      # per channel, over the frames
    y = _gelu(y.astype(dtype))
    for i in range(1, 7):
        y = _gelu(_conv1d(y, W(f"feature_extractor.conv{i}.weight"), 2))
    return np.ascontiguousarray(y.T)


def encode(w, cfg, audio, layer=None, proj=False, dtype=np.float32, pad=PAD, feats=None):
    """Hubert.encode(pad(audio), layer)[0] -> [T][n_state]; proj: HubertSoft.units -> [T][n_proj]"""
    W = lambda k: np.asarray(w[k], dtype=dtype)
    C, H, G, K = cfg["n_state"], cfg["n_head"], cfg["pos_groups"], cfg["pos_kernel"]
    x = features(w, audio, dtype, pad) if feats is None else np.asarray(feats, dtype=dtype)
    T = x.shape[0]
    x = _layer_norm(x, W("feature_projection.norm.weight"), W("feature_projection.norm.bias"))
    x = _mm(x, W("feature_projection.projection.weight").T) + W("feature_projection.projection.bias")
    # positional convolution: groups G, padding K / 2, last frame dropped
    wp = fold_weight_norm(w["positional_embedding.conv.parametrizations.weight.original0"],
                          w["positional_embedding.conv.parametrizations.weight.original1"]).astype(dtype)
    gw = C // G
    xp = np.zeros((C, T + K), dtype=dtype)
    xp[:, K // 2:K // 2 + T] = x.T
    y = np.zeros((C, T), dtype=dtype)
    for g in range(G):
        sl = slice(g * gw, (g + 1) * gw)
        cols = np.concatenate([xp[sl, k:k + T] for k in range(K)], axis=0)      # [K gw][T]
        y[sl] = _mm(np.ascontiguousarray(wp[sl].transpose(0, 2, 1)).reshape(gw, K * gw), cols)
    y = _gelu(y + W("positional_embedding.conv.bias")[:, None])
    x = _layer_norm(x + y.T, W("norm.weight"), W("norm.bias"))
    n_run = cfg["n_layer"] if layer is None else int(layer)
    D = C // H
    for l in range(n_run):
        p = f"encoder.layers.{l}."
        qkv = _mm(x, W(p + "self_attn.in_proj_weight").T) + W(p + "self_attn.in_proj_bias")
        q, k, v = (qkv[:, i * C:(i + 1) * C].reshape(T, H, D).transpose(1, 0, 2) for i in range(3))
        s = _mm(q, k.transpose(0, 2, 1)) / dtype(np.sqrt(D))
        s = s - s.max(axis=-1, keepdims=True)
        e = np.exp(s)
        a = _mm((e / e.sum(axis=-1, keepdims=True)).astype(dtype), v)
        a = a.transpose(1, 0, 2).reshape(T, C)
        x = _layer_norm(x + _mm(a, W(p + "self_attn.out_proj.weight").T) + W(p + "self_attn.out_proj.bias"), W(p + "norm1.weight"), W(p + "norm1.bias"))
        f = _gelu(_mm(x, W(p + "linear1.weight").T) + W(p + "linear1.bias"))
        x = _layer_norm(x + _mm(f, W(p + "linear2.weight").T) + W(p + "linear2.bias"), W(p + "norm2.weight"), W(p + "norm2.bias"))
    if proj:
        x = _mm(x, W("proj.weight").T) + W("proj.bias")
    return np.ascontiguousarray(x.astype(dtype))
