"""numpy restatement of the w2v-BERT 2.0 units encoder for any lds_w2vbert_cfg, in float32 or float64: the filter-bank front end
(transformers' SeamlessM4TFeatureExtractor.__call__ on one clip) and the Conformer (Wav2Vec2BertModel without adapter, position embeddings
of type "relative_key", with the extractor's attention mask).  What the CPU suite holds against the reference's fixtures and the GPU suite
against the library where no fixture exists (reduced configurations, whole outputs).  One clip at a time, as the reference runs.  Written
from the behaviour include/lds.h states; test infrastructure only."""
import numpy as np

from hubert_numpy import fixture_rows  # noqa: F401  (re-exported: the fixtures' row choice)

FIXTURE_SEED = 0
FIXTURE_LAYERS = 2
# (samples, seed) of the fixture clips: the minimum (2 frames, 1 row); odd (one valid row plus the masked row); both clamps of the distance
# and more frames than the 30-frame left context; the same with a masked row; several attention tiles
CLIPS = ((560, 158), (720, 89), (24240, 73), (24400, 74), (64240, 75))
FRAMES = (2, 3, 150, 151, 400)
ROWS = (1, 2, 75, 76, 200)
MAX_ROWS = (1, 2, 24, 24, 32)     # recorded rows per clip (the files must stay below the repository's size limit)
MIN_SAMPLES = 560
MEL_FLOOR = 1.192092955078125e-07


def frames_of(n_samples):
    """(n, valid, rows)"""
    n = 1 + (int(n_samples) - 400) // 160
    return n, n // 2, (n + 1) // 2


def make_clip(i, uniform):
    """fixture clip i: uniform noise in [-1, 1) under a slow envelope whose period (801 samples, five frames) keeps every mel bin's
    variance over time away from zero even in a two-frame clip (regenerated from the seed, never stored)"""
    n, seed = CLIPS[i]
    x = uniform(f"fix.w2vbert.clip{i}", (n,), seed, -1.0, 1.0)
    env = (0.55 + 0.45 * np.sin(np.arange(n, dtype=np.float64) * (2.0 * np.pi / 801.0) - 2.2 + 0.7 * i)).astype(np.float32)
    return (x * env).astype(np.float32)


# ---- front end -----------------------------------------------------------------------------------------------------------------------
def mel_filters(n_mels=80, n_bins=257, sr=16000):
    """Kaldi-scale triangles built in mel space, 20 Hz .. sr / 2, no normalisation -> [n_bins][n_mels]"""
    mel = lambda f: 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)
    c = np.linspace(mel(20.0), mel(sr / 2), n_mels + 2)
    fm = mel(np.arange(n_bins) * (sr / ((n_bins - 1) * 2)))[:, None]
    down = (fm - c[None, :-2]) / (c[1:-1] - c[:-2])[None]
    up = (c[None, 2:] - fm) / (c[2:] - c[1:-1])[None]
    return np.maximum(0.0, np.minimum(down, up))


def log_mel(audio, n_mels=80, like_extractor=False):
    """[n][n_mels]: the natural log of the floored Kaldi mel powers of every 400-sample frame (hop 160, not centred), float64;
    like_extractor: the spectrum rounded to complex64 on its way, as transformers' audio_utils.spectrogram stores it"""
    x = np.asarray(audio, dtype=np.float32).astype(np.float64) * 32768.0
    n = 1 + (len(x) - 400) // 160
    fr = x[np.arange(n)[:, None] * 160 + np.arange(400)[None]]
    fr = fr - fr.mean(axis=1, keepdims=True)
    pre = fr.copy()
    pre[:, 1:] -= 0.97 * fr[:, :-1]
    pre[:, 0] *= 1.0 - 0.97
    pre *= np.power(np.hanning(400), 0.85)[None]
    spec = np.fft.rfft(pre, 512, axis=1)
    if like_extractor:
        spec = spec.astype(np.complex64).astype(np.complex128)
    power = np.abs(spec) ** 2
    return np.log(np.maximum(MEL_FLOOR, power @ mel_filters(n_mels)))


def fbank(audio, n_mels=80, stride=2, dtype=np.float64):
    """input_features [rows][n_mels * stride] of one clip: normalised per mel bin over the clip's own frames (ddof = 1), padded with zeros to
    a multiple of `stride` frames, `stride` frames per row.  float64: the mathematics; float32: the extractor's own arithmetic (a complex64
    spectrum, the log-mel rounded to float32 and normalised in float32)"""
    lm = log_mel(audio, n_mels, like_extractor=dtype == np.float32)
    lm = np.ascontiguousarray(lm.T.astype(dtype)).T      # (the extractor's memory order, [bin][frame] transposed: numpy's float32 sums follow it)
    n = lm.shape[0]
    x = (lm - lm.mean(axis=0, keepdims=True)) / np.sqrt(lm.var(axis=0, ddof=1, keepdims=True) + 1e-7)
    rows = (n + stride - 1) // stride
    out = np.zeros((rows * stride, n_mels), dtype=dtype)
    out[:n] = x
    return out.reshape(rows, n_mels * stride)


# ---- model ---------------------------------------------------------------------------------------------------------------------------
def _mm(a, b):
    """a @ b with the products summed in float64 and the result rounded to the operands' type"""
    return (np.asarray(a, dtype=np.float64) @ np.asarray(b, dtype=np.float64)).astype(a.dtype)


def _layer_norm(x, g, b, eps):
    x64 = x.astype(np.float64)
    mu = x64.mean(axis=-1, keepdims=True)
    var = ((x64 - mu) ** 2).mean(axis=-1, keepdims=True)
    return (((x64 - mu) / np.sqrt(var + eps)).astype(x.dtype) * g + b).astype(x.dtype)


def _sigmoid(x):
    return (1.0 / (1.0 + np.exp(-x.astype(np.float64)))).astype(x.dtype)


def _swish(x):
    return (x * _sigmoid(x)).astype(x.dtype)


def rel_attention(q, k, v, E, valid, left, right):
    """q, k, v [H][T][64], E [left + right + 1][64] -> [H][T][64]; keys at and beyond `valid` excluded"""
    dt = q.dtype
    T = q.shape[1]
    dist = np.clip(np.arange(T)[None, :] - np.arange(T)[:, None], -left, right) + left      # [query][key]
    s = _mm(q, k.transpose(0, 2, 1)) + np.einsum("hld,lrd->hlr", q.astype(np.float64), np.asarray(E, dtype=np.float64)[dist]).astype(dt)
    s = (s / dt.type(8.0)).astype(np.float64)
    s[:, :, valid:] = -np.inf
    s = s - s.max(axis=-1, keepdims=True)
    e = np.exp(s)
    return _mm((e / e.sum(axis=-1, keepdims=True)).astype(dt), v)


def dwconv_ln_swish(x, w, g, b, eps, in_rows=None):
    """x [T][C], w [C][K] -> swish(LN_c(sum_k w[c][k] x[t - (K - 1) + k][c])); input rows at and beyond in_rows read as zeros"""
    T, C = x.shape
    K = w.shape[1]
    xp = np.zeros((T + K - 1, C), dtype=np.float64)
    xp[K - 1:] = x
    if in_rows is not None:
        xp[K - 1 + in_rows:] = 0.0
    y = np.zeros((T, C), dtype=np.float64)
    for k in range(K):
        y += xp[k:k + T] * np.asarray(w, dtype=np.float64)[None, :, k]
    return _swish(_layer_norm(y.astype(x.dtype), g, b, eps))


def encode(w, cfg, feats, n, dtype=np.float64, n_layers=None):
    """Wav2Vec2BertModel(input_features = feats [rows][n_mels * stride], attention mask of n // stride ones).last_hidden_state -> [rows][n_state]"""
    W = lambda k: np.asarray(w[k], dtype=dtype)
    C, H, eps, st = cfg["n_state"], cfg["n_head"], cfg.get("eps", 1e-5), cfg["stride"]
    left, right = cfg["left_max"], cfg["right_max"]
    x = np.asarray(feats, dtype=dtype)
    T, valid = x.shape[0], int(n) // st
    assert T == (int(n) + st - 1) // st
    x = _layer_norm(x, W("feature_projection.layer_norm.weight"), W("feature_projection.layer_norm.bias"), eps)
    x = _mm(x, W("feature_projection.projection.weight").T) + W("feature_projection.projection.bias")
    x[valid:] = 0
    for l in range(cfg["n_layer"] if n_layers is None else n_layers):
        p = f"encoder.layers.{l}."

        def ffn(x, name):
            h = _layer_norm(x, W(p + name + "_layer_norm.weight"), W(p + name + "_layer_norm.bias"), eps)
            h = _swish(_mm(h, W(p + name + ".intermediate_dense.weight").T) + W(p + name + ".intermediate_dense.bias"))
            h = _mm(h, W(p + name + ".output_dense.weight").T) + W(p + name + ".output_dense.bias")
            return (x + dtype(0.5) * h).astype(dtype)
        x = ffn(x, "ffn1")
        h = _layer_norm(x, W(p + "self_attn_layer_norm.weight"), W(p + "self_attn_layer_norm.bias"), eps)
        q, k, v = ((_mm(h, W(p + f"self_attn.linear_{c}.weight").T) + W(p + f"self_attn.linear_{c}.bias")).reshape(T, H, 64).transpose(1, 0, 2) for c in "qkv")
        a = rel_attention(q, k, v, W(p + "self_attn.distance_embedding.weight"), valid, left, right).transpose(1, 0, 2).reshape(T, C)
        x = (x + _mm(a, W(p + "self_attn.linear_out.weight").T) + W(p + "self_attn.linear_out.bias")).astype(dtype)
        h = _layer_norm(x, W(p + "conv_module.layer_norm.weight"), W(p + "conv_module.layer_norm.bias"), eps)
        h[valid:] = 0
        h = _mm(h, W(p + "conv_module.pointwise_conv1.weight")[:, :, 0].T)
        h = (h[:, :C] * _sigmoid(h[:, C:])).astype(dtype)
        h = dwconv_ln_swish(h, W(p + "conv_module.depthwise_conv.weight")[:, 0, :], W(p + "conv_module.depthwise_layer_norm.weight"),
                            W(p + "conv_module.depthwise_layer_norm.bias"), eps)
        x = (x + _mm(h, W(p + "conv_module.pointwise_conv2.weight")[:, :, 0].T)).astype(dtype)
        x = ffn(x, "ffn2")
        x = _layer_norm(x, W(p + "final_layer_norm.weight"), W(p + "final_layer_norm.bias"), eps)
    return np.ascontiguousarray(x.astype(dtype))


def encode_audio(w, cfg, audio, dtype=np.float64):
    n = frames_of(len(audio))[0]
    return encode(w, cfg, fbank(audio, cfg["n_mels"], cfg["stride"]), n, dtype)
