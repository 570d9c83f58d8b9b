"""numpy restatement of the WavLM units encoder (transformers' WavLMModel) for any lds_wavlm_cfg, in float32 or float64: what the CPU suite
holds against the fixtures recorded from WavLMModel in float64 (tests/golden/wavlm.npz) and the GPU suite against the library where no
fixture exists (the attention alone, reduced configurations).  Weights in transformers' names (lds.arch.wavlm_param_shapes).  One clip at
a time."""
import numpy as np

import hubert_numpy as hnp
from hubert_numpy import _conv1d, _gelu, _layer_norm, _mm, fixture_rows, fold_weight_norm  # noqa: F401

FIXTURE_SEED = 0
FIXTURE_LAYERS = 2
FLAVOURS = ("base", "large")      # the fixtures' two models: WavLM-Base+ and WavLM-Large at full width, FIXTURE_LAYERS blocks
# (samples, seed) of the fixture clips, hubert_numpy's generator: one frame; two frames; one frame each side of the 75 / 76 boundary (the
# last 32-key tile holds 11 / 12 keys); 350 frames (more than two 128-query blocks); 901 frames, whose distances pass max_distance = 800, so the
# saturated bucket occurs on both sides
CLIPS = ((400, 61), (720, 62), (24240, 63), (24400, 64), (112240, 65), (288400, 66))
FRAMES = (1, 2, 75, 76, 350, 901)
MAX_ROWS = (1, 2, 5, 5, 5, 6)     # recorded rows per clip (float64 rows: the file must stay below the repository's size limit)


def level_frames(n_samples):
    """frames after conv0 .. conv6 (no padding of the clip)"""
    return hnp.level_frames(n_samples, 0)


def frames_of(n_samples):
    return level_frames(n_samples)[-1]


def make_clip(i, uniform):
    """fixture clip i: hubert_numpy.make_clip's signal (uniform noise in [-1, 1) under a slow envelope) at this file's lengths, plus a
    constant offset so that the waveform normalisation has a mean to remove"""
    n, seed = CLIPS[i]
    x = uniform(f"fix.wavlm.clip{i}", (n,), seed, -1.0, 1.0)
    env = (0.55 + 0.45 * np.sin(np.arange(n, dtype=np.float64) * (2.0 * np.pi / 4001.0))).astype(np.float32)
    return (x * env * np.float32(0.5) + np.float32(0.125)).astype(np.float32)


def dims_of(flavour, arch, n_layer=FIXTURE_LAYERS):
    return dict(arch.wavlm_dims("large" if flavour == "large" else "base+"), n_layer=n_layer)


def normalize_wave(audio, dtype=np.float64):
    """Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm on one clip"""
    x = np.asarray(audio, dtype=np.float64)
    return ((x - x.mean()) / np.sqrt(x.var() + 1e-7)).astype(dtype)


def buckets(rel, num_buckets, max_distance):
    """WavLMAttention._relative_positions_bucket (rel = key - query, any integer array), the logarithm branch in float32 as torch runs it"""
    rel = np.asarray(rel, dtype=np.int64)
    nb = num_buckets // 2
    me, a = nb // 2, np.abs(rel)
    x = np.log(np.maximum(a, 1).astype(np.float32) / np.float32(me)) / np.float32(np.log(max_distance / me))
    big = np.minimum((np.float32(me) + x.astype(np.float32) * np.float32(nb - me)).astype(np.int64), nb - 1)
    return (rel > 0) * nb + np.where(a < me, a, big)


def toeplitz(embed, num_buckets, max_distance, n_ctx):
    """rel_attn_embed.weight [num_buckets][heads] -> the bias of distance d = key - query at [head][d + n_ctx - 1]"""
    b = buckets(np.arange(-(n_ctx - 1), n_ctx), num_buckets, max_distance)
    return np.ascontiguousarray(np.asarray(embed)[b].T)


def gate_of(x, w, b, const, heads):
    """x [T][C] (the attention input) -> gate [heads][T]"""
    T, C = x.shape
    p = _mm(np.ascontiguousarray(x.reshape(T, heads, C // heads).transpose(1, 0, 2)), w.T) + b      # [heads][T][8]
    s = 1.0 / (1.0 + np.exp(-p.reshape(heads, T, 2, 4).sum(-1)))
    return (s[..., 0] * (s[..., 1] * np.asarray(const).reshape(heads, 1) - 1.0) + 2.0).astype(x.dtype)


def biased_attention(q, k, v, gate, toep, n_ctx):
    """q, k, v [heads][T][64], gate [heads][T], toep [heads][2 n_ctx - 1] -> softmax(q k^T / 8 + gate[i] toep[j - i]) v, [heads][T][64]"""
    T = q.shape[1]
    idx = np.arange(T)[None, :] - np.arange(T)[:, None] + n_ctx - 1
    s = _mm(q, k.transpose(0, 2, 1)) / q.dtype.type(8.0) + gate[:, :, None] * toep[:, idx]
    s = s - s.max(axis=-1, keepdims=True)
    e = np.exp(s)
    return _mm((e / e.sum(axis=-1, keepdims=True)).astype(q.dtype), v)


def features(w, cfg, audio, dtype=np.float32):
    """feature_extractor(audio) transposed -> [T][conv_dim] (before the projection's LayerNorm)"""
    W = lambda k: np.asarray(w[k], dtype=dtype)
    y = np.asarray(audio, dtype=dtype)[None, :]
    for i in range(7):
        p = f"feature_extractor.conv_layers.{i}."
        y = _conv1d(y, W(p + "conv.weight"), 5 if i == 0 else 2)
        if cfg["stable_layer_norm"]:      # a LayerNorm over the channels of each frame behind every convolution
            y = _layer_norm(np.ascontiguousarray(y.T), W(p + "layer_norm.weight"), W(p + "layer_norm.bias")).T
        elif i == 0:                      # GroupNorm(C, C): per channel, over the frames
            y = _layer_norm(y, 1.0, 0.0).astype(dtype) * W(p + "layer_norm.weight")[:, None] + W(p + "layer_norm.bias")[:, None]
        y = _gelu(y.astype(dtype))
    return np.ascontiguousarray(y.T)


def encode(w, cfg, audio, layer=None, normalize=False, dtype=np.float32, feats=None, zero_bias=False):
    """WavLMModel(audio, output_hidden_states=True).hidden_states[layer] -> [T][n_state]; layer None = last_hidden_state"""
    W = lambda k: np.asarray(w[k], dtype=dtype)
    C, H, G, K, stable = cfg["n_state"], cfg["n_head"], cfg["pos_groups"], cfg["pos_kernel"], bool(cfg["stable_layer_norm"])
    if normalize:
        audio = normalize_wave(audio, dtype)
    x = features(w, cfg, audio, dtype) if feats is None else np.asarray(feats, dtype=dtype)
    T = x.shape[0]
    x = _layer_norm(x, W("feature_projection.layer_norm.weight"), W("feature_projection.layer_norm.bias"))
    x = _mm(x, W("feature_projection.projection.weight").T) + W("feature_projection.projection.bias")
    wp = fold_weight_norm(w["encoder.pos_conv_embed.conv.parametrizations.weight.original0"],
                          w["encoder.pos_conv_embed.conv.parametrizations.weight.original1"]).astype(dtype)
    gw = C // G
    xp = np.zeros((C, T + K), dtype=dtype)
    xp[:, K // 2:K // 2 + T] = x.T
    y = np.zeros((C, T), dtype=dtype)
    for g in range(G):
        sl = slice(g * gw, (g + 1) * gw)
        cols = np.concatenate([xp[sl, k:k + T] for k in range(K)], axis=0)      # [K gw][T]
        y[sl] = _mm(np.ascontiguousarray(wp[sl].transpose(0, 2, 1)).reshape(gw, K * gw), cols)
    x = x + _gelu(y + W("encoder.pos_conv_embed.conv.bias")[:, None]).T
    if not stable:
        x = _layer_norm(x, W("encoder.layer_norm.weight"), W("encoder.layer_norm.bias"))
    n_run = cfg["n_layer"] if layer is None else int(layer)
    toep = toeplitz(W("encoder.layers.0.attention.rel_attn_embed.weight"), cfg["num_buckets"], cfg["max_distance"], cfg["n_ctx"])
    if zero_bias:
        toep = np.zeros_like(toep)
    D = C // H
    for l in range(n_run):
        p = f"encoder.layers.{l}."
        h = _layer_norm(x, W(p + "layer_norm.weight"), W(p + "layer_norm.bias")) if stable else x
        q, k, v = ((_mm(h, W(p + f"attention.{n}_proj.weight").T) + W(p + f"attention.{n}_proj.bias")).reshape(T, H, D).transpose(1, 0, 2) for n in "qkv")
        gate = gate_of(h, W(p + "attention.gru_rel_pos_linear.weight"), W(p + "attention.gru_rel_pos_linear.bias"),
                       W(p + "attention.gru_rel_pos_const"), H)
        a = biased_attention(q, k, v, gate, toep, cfg["n_ctx"]).transpose(1, 0, 2).reshape(T, C)
        x = x + _mm(a, W(p + "attention.out_proj.weight").T) + W(p + "attention.out_proj.bias")
        if stable:
            h = _layer_norm(x, W(p + "final_layer_norm.weight"), W(p + "final_layer_norm.bias"))
        else:
            h = x = _layer_norm(x, W(p + "layer_norm.weight"), W(p + "layer_norm.bias"))
        f = _gelu(_mm(h, W(p + "feed_forward.intermediate_dense.weight").T) + W(p + "feed_forward.intermediate_dense.bias"))
        x = x + _mm(f, W(p + "feed_forward.output_dense.weight").T) + W(p + "feed_forward.output_dense.bias")
        if not stable:
            x = _layer_norm(x, W(p + "final_layer_norm.weight"), W(p + "final_layer_norm.bias"))
    if stable and n_run == cfg["n_layer"]:
        x = _layer_norm(x, W("encoder.layer_norm.weight"), W("encoder.layer_norm.bias"))
    return np.ascontiguousarray(x.astype(dtype))
