"""CTC heads without a GPU: the float64 restatement (tests/ctc_numpy.py) against torch's ctc_loss and brute force, the collapse on
planted strings, the fixture's HF loss, every refusal of the C ABI and of CTCHead (argument checks run before any device call), the
edit distance and the checkpoint helpers."""
import ctypes as C
import os

import numpy as np
import pytest

import ctc_numpy as CN
from conftest import GOLDEN

torch = pytest.importorskip("torch")

# (T, V, L, repeats planted)
CASES = ((349, 32, 60, 0), (349, 4096, 120, 0), (1499, 32, 300, 30), (7, 32, 3, 1), (3, 32, 1, 0), (1, 32, 0, 0))


def make_case(T, V, L, rep, seed=0):
    rng = np.random.default_rng(seed + T + V + L)
    z = rng.standard_normal((T, V))
    lp = z - np.log(np.exp(z).sum(axis=1, keepdims=True))
    labels = rng.integers(1, V, L)
    for k in range(rep):
        i = 1 + k * max((L - 1) // max(rep, 1), 1)
        if i < L:
            labels[i] = labels[i - 1]
    return lp, labels


def torch_ctc(lp, labels):
    T, L = lp.shape[0], len(labels)
    return float(torch.nn.functional.ctc_loss(torch.from_numpy(lp).double()[:, None], torch.from_numpy(np.asarray(labels, dtype=np.int64))[None],
                                              torch.tensor([T]), torch.tensor([L]), blank=0, reduction="none", zero_infinity=False)[0])


def test_forward_equals_torch_ctc_loss_and_fp32_sits_inside_bound_3():
    for T, V, L, rep in CASES:
        lp, labels = make_case(T, V, L, rep)
        E = CN.emissions(lp, labels, 0)
        nll, A = CN.forward(E, labels)
        ref = torch_ctc(lp, labels)
        assert abs(nll - ref) <= 1e-9 * max(1.0, abs(ref)), (T, V, L, nll, ref)
        E32 = E.astype(np.float32)
        nll64, A = CN.forward(E32, labels)
        nll32, _ = CN.forward(E32, labels, dtype=np.float32)
        assert abs(nll32 - nll64) < CN.bound3(T, A), (T, V, L)      # an fp32 numpy recursion: the a-priori probe of bound 3 (a few % of it)


def test_forward_infeasible_is_inf():
    """random labels of length 127 over 128 frames at V = 32 are infeasible by chance repeats"""
    found = 0
    for seed in range(20):
        lp, labels = make_case(128, 32, 127, 0, seed=seed)
        if CN.feasible(128, labels):
            continue
        found += 1
        assert CN.forward(CN.emissions(lp, labels, 0), labels)[0] == np.inf and torch_ctc(lp, labels) == np.inf
        assert CN.viterbi(CN.emissions(lp, labels, 0), labels)[0] == -np.inf
    assert found >= 10
    assert CN.forward(np.zeros((0, 3)), [1, 2])[0] == np.inf and CN.forward(np.zeros((0, 1)), [])[0] == 0.0


def test_viterbi_by_brute_force():
    rng = np.random.default_rng(5)
    n_tied = 0
    for i in range(150):
        T, L = int(rng.integers(1, 7)), int(rng.integers(0, 4))
        labels = rng.integers(1, 3, L)
        E = np.round(rng.standard_normal((T, L + 1)), 1 if i % 2 else 6)      # (one decimal: many exact ties)
        score, fl, seg, llp = CN.viterbi(E, labels)
        best = CN.viterbi_brute(E, labels)
        assert np.isfinite(best) == CN.feasible(T, labels)
        if not np.isfinite(best):
            assert score == -np.inf and (seg == -1).all()
            continue
        assert abs(score - best) < 1e-12 and abs(CN.path_score(E, fl) - best) < 1e-12
        assert CN.path_states_valid(fl, L) and CN.path_respects_repeats(fl, labels)
        for l in range(L):
            assert (fl[seg[l, 0]:seg[l, 1]] == l).all() and (fl == l).sum() == seg[l, 1] - seg[l, 0]
        n_tied += i % 2
    assert n_tied > 10
    # the tie rule: stay before step before skip, the final blank before the final label
    E = np.zeros((3, 2))
    assert CN.viterbi(E, [4])[1].tolist() == [0, -1, -1]      # everything ties: the path that stays the longest at the end


def test_collapse_on_planted_strings():
    c = lambda s: tuple(a.tolist() for a in CN.collapse(s, 0))
    assert c([0, 0, 0]) == ([], [], [])
    assert c([3, 3, 0, 5]) == ([3, 5], [0, 3], [2, 1])
    assert c([4, 4, 0, 4]) == ([4, 4], [0, 3], [2, 1])
    assert c([0, 0, 9]) == ([9], [2], [1])
    assert c([7]) == ([7], [0], [1]) and c([0]) == ([], [], []) and c([]) == ([], [], [])
    assert c([1, 2, 2, 1]) == ([1, 2, 1], [0, 1, 3], [1, 2, 1])
    tok, start, length, lp = CN.greedy([3, 3, 0, 5], [1.0, 3.0, 0.0, 2.0], [2.0, 5.0, 1.0, 2.5], 0)
    assert lp.tolist() == [-1.5, -0.5]


def test_fixture_hf_loss_equals_ctc_numpy(golden):
    """transformers' own loss (ctc_loss_reduction="sum", float64) on the stored labels = ctc_numpy on the stored log-probs"""
    fx = golden("ctc.npz")
    for model in ("xlsr", "wavlm"):
        for clip in (1, 2):
            lp = fx[f"{model}.clip{clip}.logprobs"].astype(np.float64)
            for L in (0, 1, 40):
                labels = fx[f"{model}.clip{clip}.labels{L}"]
                want = float(fx[f"{model}.clip{clip}.loss{L}"])
                got = CN.forward(CN.emissions(lp, labels, 0), labels)[0]
                if np.isinf(want):
                    assert got == np.inf
                else:      # the stored log-probs are rounded to fp32: u |logp| per frame
                    assert abs(got - want) <= lp.shape[0] * CN.U * np.abs(lp).max() * 2 + 1e-9, (model, clip, L, got, want)


# ---- refusals, device-free ----
@pytest.fixture(scope="module")
def lib():
    from lds import native
    return native.lib()


def _refused(lib, rc, code, *words):
    msg = lib.lds_last_error().decode()
    assert rc == code, (rc, msg)
    for w in words:
        assert w in msg, msg


def test_c_abi_refusals(lib):
    nb = C.c_size_t()
    one = (C.c_int32 * 65)(*([1] * 65))
    buf = C.create_string_buffer(1 << 16)
    p = C.cast(buf, C.c_void_p)
    # the *_workspace_bytes entries
    _refused(lib, lib.lds_ctc_head_workspace_bytes(1, 10, 32, 12, C.byref(nb)), -1, "multiple of 8")
    _refused(lib, lib.lds_ctc_head_workspace_bytes(1, 10, 1, 16, C.byref(nb)), -1, "V 1")
    _refused(lib, lib.lds_ctc_head_workspace_bytes(1, 10, 65537, 16, C.byref(nb)), -1, "V 65537")
    _refused(lib, lib.lds_ctc_head_workspace_bytes(65, 10, 32, 16, C.byref(nb)), -1, "B 65")
    _refused(lib, lib.lds_ctc_head_workspace_bytes(1, 0, 32, 16, C.byref(nb)), -1, "T 0")
    _refused(lib, lib.lds_ctc_head_workspace_bytes(64, 40000000, 32, 16, C.byref(nb)), -1, "2^31")
    _refused(lib, lib.lds_ctc_score_workspace_bytes(1, 10, 32, 16, 512, C.byref(nb)), -1, "Lmax 512")
    _refused(lib, lib.lds_ctc_align_workspace_bytes(1, 10, 32, 16, 512, C.byref(nb)), -1, "Lmax 512")
    assert lib.lds_ctc_head_workspace_bytes(2, 10, 4099, 16, C.byref(nb)) == 0 and nb.value >= 9 * 20 * 12
    assert lib.lds_ctc_score_workspace_bytes(2, 10, 32, 16, 5, C.byref(nb)) == 0
    score_bytes = nb.value
    assert lib.lds_ctc_align_workspace_bytes(2, 10, 32, 16, 5, C.byref(nb)) == 0 and nb.value >= score_bytes + 2 * 10 * 256
    align_bytes = nb.value
    # the entries themselves: every check comes before anything is enqueued (the pointers are host memory: nothing may touch them)
    head = lambda B, T, V, D, ws: lib.lds_ctc_head(p, B, T, one, p, p, V, D, p, p, p, None, p, ws, None)
    _refused(lib, head(1, 10, 32, 12, 1 << 16), -1, "multiple of 8")
    _refused(lib, head(1, 10, 1, 16, 1 << 16), -1, "V 1")
    _refused(lib, head(65, 10, 32, 16, 1 << 16), -1, "B 65")
    _refused(lib, head(2, 10, 4099, 16, 100), -2, "workspace 100 <", "bytes")
    bad_frames = (C.c_int32 * 2)(3, 11)
    _refused(lib, lib.lds_ctc_head(p, 2, 10, bad_frames, p, p, 32, 16, p, p, p, None, p, 1 << 16, None), -1, "n_frames[1] = 11")
    score = lambda V, blank, Lmax, ws, ll=one: lib.lds_ctc_score(p, 2, 10, one, p, p, V, 16, blank, p, ll, Lmax, p, p, ws, None)
    _refused(lib, score(32, 32, 5, 1 << 16), -1, "blank 32")
    _refused(lib, score(32, -1, 5, 1 << 16), -1, "blank -1")
    _refused(lib, score(32, 0, 512, 1 << 16), -1, "Lmax 512")
    _refused(lib, score(32, 0, 5, score_bytes - 1), -2, f"< {score_bytes} bytes")
    _refused(lib, score(32, 0, 5, 1 << 16, (C.c_int32 * 2)(1, 6)), -1, "label_len[1] = 6")
    align = lambda ws: lib.lds_ctc_align(p, 2, 10, one, p, p, 32, 16, 0, p, one, 5, p, p, p, p, p, ws, None)
    _refused(lib, align(align_bytes - 1), -2, f"< {align_bytes} bytes")
    _refused(lib, lib.lds_ctc_greedy(p, p, p, 65, 10, one, 0, -1, p, p, p, p, p, None), -1, "B 65")
    _refused(lib, lib.lds_ctc_greedy(p, p, None, 1, 10, one, 0, -1, p, p, p, p, p, None), -1, "null")
    _refused(lib, lib.lds_test_ctc_forward(p, 1, 10, one, p, one, 512, p, None), -1, "Lmax 512")
    _refused(lib, lib.lds_test_ctc_viterbi(p, 2, 10, one, p, one, 5, p, p, p, p, p, 2 * 10 * 256 - 1, None), -2, "5120 bytes")


def test_ctchead_refusals():
    from encoder.ctc import CTCHead
    with pytest.raises(ValueError, match="multiple of 8"):
        CTCHead(np.zeros((32, 12)), np.zeros(32))
    with pytest.raises(ValueError, match="V 1 "):
        CTCHead(np.zeros((1, 16)), np.zeros(1))
    with pytest.raises(ValueError, match="blank 32"):
        CTCHead(np.zeros((32, 16)), np.zeros(32), blank=32)
    with pytest.raises(ValueError, match=r"\[V, D\]"):
        CTCHead(np.zeros((32, 16)), np.zeros(31))
    head = CTCHead.synthetic(16, 32, seed=1, blank=0)
    units = torch.zeros(2, 10, 16)
    for call in (lambda: head.log_probs(units, [10, 3]), lambda: head.greedy(units, [10, 3]), lambda: head.score(units, [10, 3], [[1], [2]]),
                 lambda: head.align(units, [10, 3], [[1], [2]])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    # a blank or out-of-range label is refused before anything is uploaded (CPU units: the label check comes first)
    with pytest.raises(ValueError, match="blank"):
        head.score(units, [10, 3], [[1, 0], [2]])
    with pytest.raises(ValueError, match="outside 0 .. 31"):
        head.align(units, [10, 3], [[1, 32], [2]])
    with pytest.raises(ValueError, match="outside 0 .. 31"):
        head.score(units, [10, 3], [[-1], [2]])
    with pytest.raises(ValueError, match="at most 511"):
        head.score(units, [10, 3], [[1] * 512, [2]])
    with pytest.raises(ValueError, match="transcripts for 2 clips"):
        head.score(units, [10, 3], [[1]])
    with pytest.raises(ValueError, match="vocab"):
        head.decode([1, 2])


def test_ctchead_refuses_units_that_are_not_the_last_hidden_state():
    from encoder.ctc import CTCHead

    class Stack:
        dims = {"n_layer": 12}

    class Soft:          # HubertUnits('hubertsoft'): proj is set
        proj, model = True, Stack()

    class ContentVec:    # HubertUnits('contentvec768l12')
        proj, model = False, Stack()

    class Wav:           # WavLMUnits
        def __init__(self, layer):
            self.units_layer, self.model = layer, Stack()

    with pytest.raises(ValueError, match="hubertsoft"):
        CTCHead.check_source(Soft())
    with pytest.raises(ValueError, match="units_layer"):
        CTCHead.check_source(Wav(6))
    CTCHead.check_source(ContentVec())
    CTCHead.check_source(Wav(12))
    # the real classes carry those attributes
    from tools.tools import HubertUnits, WavLMUnits
    from lds import arch
    dims = dict(arch.HUBERT_BASE_DIMS, n_layer=1)
    with pytest.raises(ValueError, match="hubertsoft"):
        CTCHead.check_source(HubertUnits.synthetic("hubertsoft", dims=dims, device="cpu"))
    CTCHead.check_source(HubertUnits.synthetic("contentvec768l12", dims=dims, device="cpu"))
    wd = dict(arch.wavlm_dims("base+"), n_layer=2)
    with pytest.raises(ValueError, match="units_layer"):
        CTCHead.check_source(WavLMUnits.synthetic(dims=wd, device="cpu", units_layer=1))
    CTCHead.check_source(WavLMUnits.synthetic(dims=wd, device="cpu"))


def test_edit_distance():
    from encoder.ctc import edit_distance
    for f in (edit_distance, CN.edit_distance):
        assert f("kitten", "sitting") == 3 and f([], []) == 0 and f([1, 2, 3], []) == 3 and f([], [4]) == 1
        assert f([1, 2, 3], [1, 2, 3]) == 0 and f([1, 2, 3], [1, 3]) == 1 and f("flaw", "lawn") == 2


def test_checkpoint_helpers(tmp_path):
    """load_ctc_encoder_state on a synthetic prefixed dict; CTCHead.from_checkpoint with config.json and vocab.json next to it"""
    import json
    from encoder.ctc import CTCHead, load_ctc_encoder_state
    enc = {"feature_projection.projection.weight": torch.ones(4, 3), "encoder.layers.0.attention.k_proj.bias": torch.zeros(4)}
    for prefix in ("wav2vec2.", "wavlm.", "hubert."):
        full = {prefix + k: v for k, v in enc.items()}
        full["lm_head.weight"], full["lm_head.bias"] = torch.arange(40 * 16, dtype=torch.float32).reshape(40, 16), torch.arange(40, dtype=torch.float32)
        got = load_ctc_encoder_state(full)
        assert set(got) == set(enc) and all(torch.equal(got[k], enc[k]) for k in enc)
    with pytest.raises(ValueError, match="more than one"):
        load_ctc_encoder_state({"wav2vec2.a": torch.zeros(1), "hubert.b": torch.zeros(1)})
    torch.save(full, tmp_path / "pytorch_model.bin")
    json.dump({"pad_token_id": 39, "vocab_size": 40}, open(tmp_path / "config.json", "w"))
    json.dump({"a": 1, "b": 2, "|": 3, "<pad>": 39}, open(tmp_path / "vocab.json", "w"))
    assert set(load_ctc_encoder_state(tmp_path / "pytorch_model.bin")) == set(enc)
    head = CTCHead.from_checkpoint(tmp_path / "pytorch_model.bin")
    assert (head.V, head.D, head.blank) == (40, 16, 39) and head.decode([1, 2, 3, 2, 1]) == "ab ba"
    from safetensors.torch import save_file
    save_file({k: v.contiguous() for k, v in full.items()}, str(tmp_path / "model.safetensors"))
    h2 = CTCHead.from_checkpoint(tmp_path / "model.safetensors")
    assert torch.equal(h2._w, head._w) and torch.equal(h2._b, head._b) and h2.blank == 39
    with pytest.raises(ValueError, match="lm_head"):
        torch.save(enc, tmp_path / "enc.bin")
        CTCHead.from_checkpoint(tmp_path / "enc.bin")
