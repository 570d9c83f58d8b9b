"""numpy restatement of the x-vector speaker head (transformers 5.15 modeling_wavlm.py: TDNNLayer, WavLMForXVector.forward without an
attention_mask) in float64, and the a-priori bounds the GPU suite holds csrc/xvector.hip to.  One clip at a time; weights under the
head's transformers names.  The CPU suite holds it against the fixtures recorded from WavLMForXVector in float64 (tests/golden/xvector.npz).

Bounds (u = 2^-24, the unit round-off of fp32):
  1  one output of a layer.  y = b + sum of K = ks Cin products formed as one fmaf chain in fp32: the chain's error is at most
     K u sum|x||w| (one rounding per step on a partial sum below sum|x||w|, to first order), adding the bias rounds once more, and
     (1 + u)^(K + 1) - 1 <= (K + 3) u for K u < 0.01 covers the higher orders: |y - y64| <= (K + 3) u (sum|x||w| + |b|).  ReLU does not
     increase a difference.
  2  the layer sum.  out = sum_l w_l h_l as n_layer + 1 fmaf steps: (n_layer + 2) u sum_l |w_l h_l| by the same argument.
  3  the cosine.  Numerator and both squared norms are dim-term sums of products: each within dim u of its sum of absolute values (any
     order), and |a.b| <= |a||b|; the two square roots, the product and the quotient round once each: |c - c64| <= (dim + 4) u.
The pooling is held to relative bounds on (mean, M2) against the float64 statistics of the kernel's own fp32 output (mean 1e-5, M2 1e-3:
what tests/test_gpu_wino_modes.py holds the same combination of partials to)."""
import numpy as np

U = 2.0 ** -24
DEFAULT = dict(tdnn_dim=(512, 512, 512, 512, 1500), tdnn_kernel=(5, 3, 3, 1, 1), tdnn_dilation=(1, 2, 3, 1, 1), xvector_output_dim=512)


# the fixtures (tests/golden/xvector.npz): three 2-layer WavLMForXVector models on four clips, each clip alone
MODELS = ("base_sum", "base_last", "large_last")      # Base with / without the weighted layer sum; Large (stable, every clip normalised)
SHORT_CLIPS = ((5200, 71), (5520, 72))                # (samples, seed): 16 frames = the shortest clip the head takes (T_out 2), and 17
WAVLM_CLIPS = (2, 4)                                  # wavlm_numpy's clips of 75 and 350 frames
FRAMES = (16, 17, 75, 350)
N_LABELS = 512      # HF's classifier is Linear(xvector_output_dim, xvector_output_dim); num_labels sizes the training objective only
HEAD_SEED = 0


def make_clips(wnp, uniform):
    """the four fixture clips, regenerated from seeds (never stored): wavlm_numpy.make_clip's signal at the two short lengths, then its clips"""
    out = []
    for i, (n, seed) in enumerate(SHORT_CLIPS):
        x = uniform(f"fix.xvector.clip{i}", (n,), seed, -1.0, 1.0)
        env = (0.55 + 0.45 * np.sin(np.arange(n, dtype=np.float64) * (2.0 * np.pi / 4001.0))).astype(np.float32)
        out.append((x * env * np.float32(0.5) + np.float32(0.125)).astype(np.float32))
    return out + [wnp.make_clip(i, uniform) for i in WAVLM_CLIPS]


def f64(a):
    return np.asarray(a, dtype=np.float64)


def softmax(w):
    w = f64(w)
    e = np.exp(w - w.max())
    return e / e.sum()


def layer_sum(hidden_states, layer_weights):
    """hidden_states: n_layer + 1 arrays [T, D]; layer_weights raw (soft-maxed here)"""
    w = softmax(layer_weights)
    return sum(w[l] * f64(h) for l, h in enumerate(hidden_states))


def unfold(x, ks, dil):
    """x [T, Cin] -> [T_out, ks Cin], tap-major: row t = x[t], x[t + d], .., x[t + (ks - 1) d]"""
    x = f64(x)
    t_out = x.shape[0] - (ks - 1) * dil
    if t_out <= 0:
        return np.zeros((0, ks * x.shape[1]))
    return np.concatenate([x[j * dil:j * dil + t_out] for j in range(ks)], axis=1)


def tdnn(x, W, b, ks, dil, relu=True):
    """x [T, Cin], W [Cout, ks Cin] (tdnn.{i}.kernel.weight as stored), b [Cout] -> [T - (ks - 1) dil, Cout]"""
    y = unfold(x, ks, dil) @ f64(W).T + f64(b)
    return np.maximum(y, 0.0) if relu else y


def delta_tdnn(x, W, b, ks, dil):
    """bound 1, [T_out, Cout]"""
    K = ks * np.asarray(x).shape[1]
    return (K + 3) * U * (np.abs(unfold(x, ks, dil)) @ np.abs(f64(W)).T + np.abs(f64(b))[None, :])


def pool(y):
    """[T_out, C] -> [2 C]: means, then torch.std (ddof 1)"""
    y = f64(y)
    if y.shape[0] < 2:
        raise ValueError(f"pooling needs 2 frames (got {y.shape[0]})")
    return np.concatenate([y.mean(axis=0), y.std(axis=0, ddof=1)])


def pool_m2(y):
    """[T_out, C] -> (mean [C], M2 [C])"""
    y = f64(y)
    m = y.mean(axis=0)
    return m, ((y - m) ** 2).sum(axis=0)


def head(state, hidden, geometry=None):
    """the head on one clip: hidden [T, D] -> (embeddings [xvector_dim], logits [n_labels])"""
    g = dict(DEFAULT, **(geometry or {}))
    x = f64(hidden) @ f64(state["projector.weight"]).T + f64(state["projector.bias"])
    for i, (ks, dil) in enumerate(zip(g["tdnn_kernel"], g["tdnn_dilation"])):
        x = tdnn(x, state[f"tdnn.{i}.kernel.weight"], state[f"tdnn.{i}.kernel.bias"], ks, dil)
    emb = f64(state["feature_extractor.weight"]) @ pool(x) + f64(state["feature_extractor.bias"])
    return emb, f64(state["classifier.weight"]) @ emb + f64(state["classifier.bias"])


def cosine(a, b, eps=1e-8):
    """a [N, dim], b [M, dim] -> [N, M]: torch.nn.functional.cosine_similarity of every pair"""
    a, b = f64(a), f64(b)
    return (a @ b.T) / (np.maximum(np.linalg.norm(a, axis=1), eps)[:, None] * np.maximum(np.linalg.norm(b, axis=1), eps)[None, :])


def delta_layer_sum(hidden_states, w):
    """bound 2; w already soft-maxed"""
    return (len(hidden_states) + 1) * U * sum(np.abs(f64(w[l]) * f64(h)) for l, h in enumerate(hidden_states))


def delta_cosine(dim):
    """bound 3"""
    return (dim + 4) * U
