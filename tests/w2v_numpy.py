"""numpy restatement of the wav2vec 2.0 units encoder in its layer-norm flavour (XLSR-53) for any lds_w2v_cfg, in float32 or float64:
what the CPU suite holds against transformers.Wav2Vec2Model's fixtures and the GPU suite against the library where no fixture exists
(every frame of the long clips, reduced configurations).  Weights in fairseq's names (lds.arch.w2v_param_shapes).  One clip at a time."""
import numpy as np

import hubert_numpy as hnp
from hubert_numpy import _gelu, _layer_norm, _mm, fixture_rows, fold_weight_norm  # noqa: F401

FIXTURE_SEED = 0
FIXTURE_LAYERS = 2
# (samples, seed) of the fixture clips: hubert_numpy's generator and seeds; the shortest clip the encoder takes (1 frame), floors that
# drop frames, the positional kernel's width, a 64-frame tile boundary and a whole 128-tap window inside, and a frame count that is a
# multiple of neither 4 nor 32 with more than 64 + 127 frames
CLIPS = ((400, 51), (1279, 52), (41277, 53), (61760, 54), (112077, 55))
FRAMES = (1, 3, 128, 192, 349)
MAX_ROWS = (1, 3, 24, 24, 32)     # recorded rows per clip (the file must stay below the repository's size limit)


def level_frames(n_samples):
    """frames after conv0 .. conv6 (no padding of the clip)"""
    return hnp.level_frames(n_samples, 0)


def frames_of(n_samples):
    return level_frames(n_samples)[-1]


def make_clip(i, uniform):
    """fixture clip i: hubert_numpy.make_clip's signal (uniform noise in [-1, 1) under a slow envelope) at this file's lengths"""
    n, seed = CLIPS[i]
    x = uniform(f"fix.hubert.clip{i}", (n,), seed, -1.0, 1.0)
    env = (0.55 + 0.45 * np.sin(np.arange(n, dtype=np.float64) * (2.0 * np.pi / 4001.0))).astype(np.float32)
    return (x * env).astype(np.float32)


def _conv1d(x, w, b, stride):
    """x [Ci][T], w [Co][Ci][K], b [Co], no padding -> [Co][To]"""
    Co, Ci, K = w.shape
    To = (x.shape[1] - K) // stride + 1
    cols = np.concatenate([np.ascontiguousarray(x[:, k:k + stride * (To - 1) + 1:stride]) for k in range(K)], axis=0)      # [K Ci][To]
    return _mm(np.ascontiguousarray(w.transpose(0, 2, 1)).reshape(Co, K * Ci), cols) + b[:, None]


def ln_act(x, g, b, eps=1e-5):
    """x [C][T] -> GELU(LayerNorm over the channels of each frame)"""
    return _gelu(_layer_norm(np.ascontiguousarray(x.T), g, b, eps)).T


def features(w, audio, dtype=np.float32):
    """the feature extractor -> [T][conv_dim] (after the last LayerNorm + GELU, before the projection's LayerNorm)"""
    W = lambda k: np.asarray(w[k], dtype=dtype)
    y = np.asarray(audio, dtype=dtype)[None, :]
    for i in range(7):
        p = f"feature_extractor.conv_layers.{i}."
        y = _conv1d(y, W(p + "0.weight"), W(p + "0.bias"), 5 if i == 0 else 2)
        y = ln_act(y, W(p + "2.1.weight"), W(p + "2.1.bias"))
    return np.ascontiguousarray(y.T)


def encode(w, cfg, audio, dtype=np.float32, feats=None):
    """extract_features(audio, padding_mask=all False)["x"] -> [T][n_state]"""
    W = lambda k: np.asarray(w[k], dtype=dtype)
    C, H, G, K = cfg["n_state"], cfg["n_head"], cfg["pos_groups"], cfg["pos_kernel"]
    x = features(w, audio, dtype) if feats is None else np.asarray(feats, dtype=dtype)
    T = x.shape[0]
    x = _layer_norm(x, W("layer_norm.weight"), W("layer_norm.bias"))
    x = _mm(x, W("post_extract_proj.weight").T) + W("post_extract_proj.bias")
    # positional convolution: groups G, padding K / 2, last frame dropped; no LayerNorm behind it
    wp = fold_weight_norm(w["encoder.pos_conv.0.weight_g"], w["encoder.pos_conv.0.weight_v"]).astype(dtype)
    gw = C // G
    xp = np.zeros((C, T + K), dtype=dtype)
    xp[:, K // 2:K // 2 + T] = x.T
    y = np.zeros((C, T), dtype=dtype)
    for g in range(G):
        sl = slice(g * gw, (g + 1) * gw)
        cols = np.concatenate([xp[sl, k:k + T] for k in range(K)], axis=0)      # [K gw][T]
        y[sl] = _mm(np.ascontiguousarray(wp[sl].transpose(0, 2, 1)).reshape(gw, K * gw), cols)
    x = x + _gelu(y + W("encoder.pos_conv.0.bias")[:, None]).T
    D = C // H
    for l in range(cfg["n_layer"]):
        p = f"encoder.layers.{l}."
        h = _layer_norm(x, W(p + "self_attn_layer_norm.weight"), W(p + "self_attn_layer_norm.bias"))
        q, k, v = ((_mm(h, W(p + f"self_attn.{n}_proj.weight").T) + W(p + f"self_attn.{n}_proj.bias")).reshape(T, H, D).transpose(1, 0, 2) for n in "qkv")
        s = _mm(q, k.transpose(0, 2, 1)) / dtype(np.sqrt(D))
        s = s - s.max(axis=-1, keepdims=True)
        e = np.exp(s)
        a = _mm((e / e.sum(axis=-1, keepdims=True)).astype(dtype), v).transpose(1, 0, 2).reshape(T, C)
        x = x + _mm(a, W(p + "self_attn.out_proj.weight").T) + W(p + "self_attn.out_proj.bias")
        h = _layer_norm(x, W(p + "final_layer_norm.weight"), W(p + "final_layer_norm.bias"))
        f = _gelu(_mm(h, W(p + "fc1.weight").T) + W(p + "fc1.bias"))
        x = x + _mm(f, W(p + "fc2.weight").T) + W(p + "fc2.bias")
    x = _layer_norm(x, W("encoder.layer_norm.weight"), W("encoder.layer_norm.bias"))
    return np.ascontiguousarray(x.astype(dtype))
