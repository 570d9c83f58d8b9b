"""Teacher-forced Llama scoring and prompted generation without a GPU: the numpy restatement (tests/llama_score_numpy.py over
tests/llama_numpy.py's cached decoder) against the reference's own `forward` recorded in tests/golden/llama_score.npz, the id and stream
arithmetic of `Llama.score`, every new refusal, `semantic_prompt` no longer swallowed, the C ABI's new names, and lds_llama_score's limits,
which answer before any device call."""
import ctypes as ct
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

import llama_score_numpy as LS

LOGITS_TOL = 2e-5      # the project's LM logits bound; lp / loss: eps = 2 * LOGITS_TOL * absmax (log-sum-exp is 1-Lipschitz in the max norm)
CASES = [("greedy", 0), ("greedy", 1), ("random", 0), ("random", 1)]


@pytest.fixture(scope="module")
def fx():
    f = dict(np.load(os.path.join(GOLDEN, "llama.npz")))
    f["toy"] = json.loads(bytes(f["toy_json"]).decode())
    return f


@pytest.fixture(scope="module")
def sx():
    return dict(np.load(os.path.join(GOLDEN, "llama_score.npz")))


@pytest.fixture(scope="module")
def toy(fx):
    from lds import arch
    t = dict(fx["toy"])
    cfg = arch.llama_config(semantic_kmeans_num=t.pop("semantic_kmeans_num"), **t)
    return cfg, arch.llama_init_state(cfg, int(fx["weight_seed"]))


@pytest.fixture(scope="module")
def model(fx):
    from text2semantic.llama.llama import Llama
    t = dict(fx["toy"])
    return Llama(t, semantic_kmeans_num=t.pop("semantic_kmeans_num"), codebook_path="/nonexistent")


def pinned(logits, labels, eps):
    """position t is pinned when no other reference logit lies within eps of the label's"""
    out = np.zeros(len(labels) - 1, bool)
    for t in range(len(labels) - 1):
        y = int(labels[t + 1])
        if y >= 0:
            out[t] = np.abs(np.delete(logits[t], y) - logits[t, y]).min() > eps
    return out


@pytest.mark.parametrize("case,b", CASES)
def test_restatement_reproduces_the_reference_forward(fx, sx, toy, case, b):
    cfg, state = toy
    p = f"{case}_r{b}_"
    ids, ref = sx[p + "ids"], sx[p + "logits"]
    assert np.array_equal(ids, LS.stream(cfg, fx[f"phone_r{b}"], sx[p + "semantic"], append_eos=True))
    lp, rank, loss, n, logits = LS.score_ids(state, cfg, fx["inv_freq"], ids[None])
    eps = 2 * LOGITS_TOL * float(np.abs(ref).max())
    rel = float(np.abs(logits[0] - ref).max() / np.abs(ref).max())
    pin = pinned(ref, ids, eps)
    print(f"{case} r{b}: logits relmax {rel:.3e}, lp err {np.abs(lp[0] - sx[p + 'lp']).max():.3e} (eps {eps:.3e}), pinned {pin.sum()}/{len(pin)}")
    assert rel < LOGITS_TOL and n == len(ids) - 1
    assert np.abs(lp[0] - sx[p + "lp"]).max() < eps and abs(loss - float(sx[p + "loss"])) < eps
    assert pin.sum() >= 0.9 * len(pin) and np.array_equal(rank[0][pin], sx[p + "rank"][pin])


def test_restatement_reproduces_the_batched_loss(fx, sx, toy):
    cfg, state = toy
    ids, mask, labels = sx["batch_ids"], sx["batch_mask"], sx["batch_labels"]
    lp, rank, loss, n, _ = LS.score_ids(state, cfg, fx["inv_freq"], ids, mask.sum(1), labels)
    eps = 2 * LOGITS_TOL * max(float(np.abs(sx[f"random_r{b}_logits"]).max()) for b in range(2))
    assert n == int(sx["batch_n"]) and abs(loss - float(sx["batch_loss"])) < eps
    assert np.array_equal(rank >= 0, labels[:, 1:] >= 0)


def test_fixture_holds_what_the_recipe_states(fx, sx):
    assert [len(sx[f"greedy_r{b}_ids"]) for b in range(2)] == [49, 49] and [len(sx[f"random_r{b}_ids"]) for b in range(2)] == [57, 49]
    for b in range(2):
        assert np.array_equal(sx[f"greedy_r{b}_semantic"], fx[f"greedy_r{b}_tokens"]) and len(sx[f"random_r{b}_semantic"]) == 30
        assert sx[f"greedy_r{b}_logits"].shape == (49, 172)
    assert sx["batch_mask"].sum(1).tolist() == [57, 49] and (sx["batch_labels"][1, 49:] == -100).all() and (sx["batch_labels"][1, [20, 21, 33]] == -100).all()
    assert int(sx["batch_n"]) == 56 + 48 - 3
    assert os.path.getsize(os.path.join(GOLDEN, "llama_score.npz")) < 256 * 1024


def test_score_stream_arithmetic(model):
    m, K = model, model.cfg["semantic_kmeans_num"]
    bos, eos, pad = 108 + K, 108 + K + 1, 108 + K + 2
    ph = torch.tensor([[5, 6, 7, 0], [9, 8, 0, 0]])
    mask = torch.tensor([[1, 1, 1, 0], [1, 1, 0, 0]])
    sem = torch.tensor([[3, 4, K + 1, K + 2, K + 2], [1, 2, 3, 4, 5]])      # row 0 ends behind its EOS, row 1 runs to the end
    assert m.semantic_lengths(sem) == [3, 5] and m.semantic_lengths(torch.tensor([[3, K + 2, K + 1]])) == [1]
    assert m.semantic_lengths(sem, torch.tensor([[1, 1, 1, 1, 0], [1, 1, 0, 0, 0]])) == [4, 2]
    ids, lens, lab, at, valid = m.score_streams(ph, sem, mask)
    assert ids.tolist() == [[108, 5, 6, 7, 109, bos, 111, 112, eos, pad], [108, 9, 8, 109, bos, 109, 110, 111, 112, 113]] and lens == [9, 10]
    assert lab.tolist() == [[-100] * 6 + [111, 112, eos, -100], [-100] * 5 + [109, 110, 111, 112, 113]]      # the semantic targets only
    assert valid.tolist() == [[True, True, True, False, False], [True] * 5]
    assert at[0, :3].tolist() == [5, 6, 7] and at[1].tolist() == [4, 5, 6, 7, 8]      # the position that predicts token j: one before its id
    for b in range(2):
        for j in range(5):
            if valid[b, j]:
                assert ids[b, at[b, j] + 1] == sem[b, j] + 108
    # append_eos: the reference forward's stream (llama.py:98-101), the EOS a target of its own
    ids, lens, lab, at, valid = m.score_streams(ph[1:, :2], sem[1:], append_eos=True)
    assert ids.tolist() == [[108, 9, 8, 109, bos, 109, 110, 111, 112, 113, eos]] and lens == [11] and at.tolist() == [[4, 5, 6, 7, 8, 9]]
    assert lab.tolist() == [[-100] * 5 + [109, 110, 111, 112, 113, eos]] and bool(valid.all())
    # "stream": labels = input_ids, every id of the stream
    ids2, lens2, lab2, at2, _ = m.score_streams(ph[1:, :2], sem[1:], append_eos=True, labels="stream")
    assert lab2 is None and torch.equal(ids2, ids) and torch.equal(at2, at)
    # a [B, T] tensor with holes
    given = torch.tensor([[3, -100, K + 1, 0, 0], [-100, 2, 3, 4, 5]])
    _, _, lab3, _, _ = m.score_streams(ph, sem, mask, labels=given)
    assert lab3.tolist() == [[-100] * 6 + [111, -100, eos, -100], [-100] * 6 + [110, 111, 112, 113]]
    # the generate prompt's stream: [108, phones, 109, prompt + 108], every row with its own length
    tails = m._check_prompt(2, torch.tensor([[K, 7, 8], [K, 9, 0]]), torch.tensor([[1, 1, 1], [1, 1, 0]]))
    ids, lens, nph = m._streams(ph, mask, tails)
    assert ids.tolist() == [[108, 5, 6, 7, 109, bos, 115, 116], [108, 9, 8, 109, bos, 117, pad, pad]] and lens == [8, 6] and nph == [3, 2]


def test_new_refusals(model):
    from text2semantic.roformer.roformer import LMScore
    m, K = model, model.cfg["semantic_kmeans_num"]
    assert list(inspect.signature(m.score).parameters) == ["phone", "tone", "semantic", "attention_mask", "semantic_attention_mask", "labels", "append_eos",
                                                          "return_logits"]
    assert list(inspect.signature(m.score_ids).parameters) == ["input_ids", "attention_mask", "labels", "return_logits"]
    assert LMScore._fields == ("loss", "token_logprobs", "ranks", "seq_logprob", "n_tokens", "logits")
    ph, sem = torch.tensor([[1, 2, 3]]), torch.tensor([[4, 5, 6, 7]])
    ids = torch.tensor([[108, 1, 2, 109, 108 + K, 112]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.score(ph, ph, sem)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.score_ids(ids)
    with pytest.raises(ValueError, match="semantic"):
        m.score(ph, ph, torch.ones(2, 4, dtype=torch.long))
    with pytest.raises(ValueError, match="semantic ids"):
        m.score(ph, ph, torch.tensor([[4, K + 3, 6, 7]]))
    with pytest.raises(ValueError, match="semantic ids"):
        m.score(ph, ph, torch.tensor([[4, -1, 6, 7]]))
    with pytest.raises(ValueError, match="no semantic token"):
        m.score(ph, ph, torch.tensor([[K + 2, 1, 2]]))
    with pytest.raises(ValueError, match="labels"):
        m.score(ph, ph, sem, labels="all")
    with pytest.raises(ValueError, match="labels"):
        m.score(ph, ph, sem, labels=torch.ones(1, 5, dtype=torch.long))
    with pytest.raises(ValueError, match="labels"):
        m.score(ph, ph, sem, labels=torch.tensor([[4, K + 3, 6, 7]]))
    with pytest.raises(NotImplementedError, match="right-padded"):
        m.score(ph, ph, sem, semantic_attention_mask=torch.tensor([[1, 0, 1, 1]]))
    with pytest.raises(NotImplementedError, match="right-padded"):
        m.score(ph, ph, sem, attention_mask=torch.tensor([[0, 1, 1]]))
    with pytest.raises(ValueError, match="max_position_embeddings"):
        m.score(ph, ph, torch.ones(1, 124, dtype=torch.long))      # 3 + 3 + 124 > 128
    with pytest.raises(ValueError, match="S"):
        m.score_ids(ids[:, :1])
    with pytest.raises(ValueError, match="S"):
        m.score_ids(torch.ones(1, 129, dtype=torch.long))
    with pytest.raises(ValueError, match="labels"):
        m.score_ids(ids, labels=ids[:, :5])
    with pytest.raises(NotImplementedError, match="right-padded"):
        m.score_ids(ids, attention_mask=torch.tensor([[1, 1, 0, 1, 1, 1]]))
    with pytest.raises(ValueError, match="input_ids inside"):
        m.score_ids(torch.tensor([[108, 1, 2, 109, 108 + K + 3, 112]]))
    with pytest.raises(ValueError, match="input_ids inside"):
        m.score_ids(torch.tensor([[108, -1, 2, 109, 108 + K, 112]]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # ... but whatever sits behind a row's length is not looked at
        m.score_ids(torch.tensor([[108, 1, 2, 109, 108 + K, 10 ** 9]]), attention_mask=torch.tensor([[1, 1, 1, 1, 1, 0]]))
    with pytest.raises(ValueError, match="labels inside"):
        m.score_ids(ids, labels=torch.tensor([[108, 1, 2, 109, 108 + K, 10 ** 9]]))
    # what stays out of scope keeps raising
    with pytest.raises(NotImplementedError, match="training"):
        m(ph, ph, sem, labels=sem)
    with pytest.raises(NotImplementedError, match="beam"):
        m.generate(ph, ph, num_beams=2, max_length=16, semantic_prompt=torch.tensor([[K, 1]]))


def test_semantic_prompt_is_not_swallowed(model):
    m, K = model, model.cfg["semantic_kmeans_num"]
    par = inspect.signature(m.generate).parameters
    assert "semantic_prompt" in par and "prompt_attention_mask" in par and par["semantic_prompt"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    ph = torch.tensor([[1, 2, 3]])
    with pytest.raises(ValueError, match="BOS"):
        m.generate(ph, ph, max_length=16, semantic_prompt=torch.tensor([[5, 6]]))
    with pytest.raises(ValueError, match="prompt ids"):
        m.generate(ph, ph, max_length=16, semantic_prompt=torch.tensor([[K, K + 3]]))
    with pytest.raises(ValueError, match="prompt ids"):
        m.generate(ph, ph, max_length=16, semantic_prompt=torch.tensor([[K, -1]]))
    with pytest.raises(ValueError, match="semantic_prompt must be"):
        m.generate(ph, ph, max_length=16, semantic_prompt=torch.tensor([K, 1]))
    with pytest.raises(ValueError, match="semantic_prompt must be"):
        m.generate(ph, ph, max_length=16, semantic_prompt=torch.tensor([[K, 1], [K, 2]]))
    with pytest.raises(ValueError, match="prompt_attention_mask"):
        m.generate(ph, ph, max_length=16, prompt_attention_mask=torch.tensor([[1, 1]]))
    with pytest.raises(ValueError, match="prompt_attention_mask"):
        m.generate(ph, ph, max_length=16, semantic_prompt=torch.tensor([[K, 1]]), prompt_attention_mask=torch.tensor([[1, 1, 1]]))
    with pytest.raises(NotImplementedError, match="right-padded"):
        m.generate(ph, ph, max_length=16, semantic_prompt=torch.tensor([[K, 1, 2]]), prompt_attention_mask=torch.tensor([[1, 0, 1]]))
    with pytest.raises(ValueError, match="BOS"):
        m.generate(ph, ph, max_length=16, semantic_prompt=torch.tensor([[K, 1, 2]]), prompt_attention_mask=torch.tensor([[0, 0, 0]]))
    # max_length counts everything: 6 ids of [108, phones, 109, BOS] and 10 prompt tokens leave no room below 16 ...
    prompt = torch.cat([torch.tensor([[K]]), torch.arange(10)[None]], dim=1)
    with pytest.raises(ValueError, match="10 prompt tokens"):
        m.generate(ph, ph, max_length=16, semantic_prompt=prompt)
    with pytest.raises(RuntimeError, match="HIP device"):      # ... and room below 17: the call gets as far as the device
        m.generate(ph, ph, max_length=17, semantic_prompt=prompt)


def test_abi_entries_declared():
    from lds import native
    hdr = open(os.path.join(ROOT, "include", "lds.h")).read()
    for name, kinds in (("lds_llama_score_workspace_bytes", "piip"), ("lds_llama_score", "ppppiippppppzp")):
        assert f"int  {name}(" in hdr and name in native.EXPORTS and native.SIGNATURES[name] == "i:" + kinds
        decl = hdr[hdr.index(f"int  {name}("):]
        decl = decl[: decl.index(";")]
        args = [a.strip() for a in decl[decl.index("(") + 1: decl.rindex(")")].split(",")]
        want = "".join("p" if "*" in a else "z" if a.startswith("size_t") else "i" for a in args)
        assert want == kinds, (name, want)
    doc = hdr[hdr.index("Teacher-forced scoring under the Llama"): hdr.index("int  lds_llama_score_workspace_bytes(")]
    assert "llama.py:73-117" in doc and "dataloader.py:182-183" in doc
    assert hasattr(native.Llama, "score")
    if os.path.exists(native.LIB_PATH):
        L = native.lib()
        assert hasattr(L, "lds_llama_score") and hasattr(L, "lds_llama_score_workspace_bytes")


def test_score_limits_answer_before_any_device_call():
    """B, S and B * S are checked before the handle, the model's positions before anything touches a device: they answer on a machine without one"""
    from lds import native
    L = native.lib()
    nb = ct.c_size_t(77)

    def score(B, S):
        return L.lds_llama_score(None, None, None, None, B, S, None, None, None, None, None, None, 0, None)

    for B, S, word in ((0, 8, b"B >= 1"), (-3, 8, b"B >= 1"), (1, 1, b"2 .."), (1, 0, b"2 .."), (1, 15001, b"15000"), (35, 15000, b"524280"), (65536, 8, b"524280"),
                       (2, 8, b"null handle")):
        assert score(B, S) == -1 and word in L.lds_last_error(), (B, S, L.lds_last_error())
        assert L.lds_llama_score_workspace_bytes(None, B, S, ct.byref(nb)) == -1 and word in L.lds_last_error() and nb.value == 77
    assert score(34, 15000) == -1 and b"null handle" in L.lds_last_error()      # 510000 rows pass the batch limit


def test_tools_argument_parsing():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import infer_tts
    import validate_lm
    assert validate_lm.parse_args(["--synthetic"]).lm_type == "roformer" and validate_lm.parse_args(["--synthetic", "--lm_type", "llama"]).lm_type == "llama"
    assert callable(validate_lm.validate_llama) and callable(infer_tts.text2semantic_llama_candidates)
    assert "semantic_prompt" in inspect.signature(infer_tts.text2semantic_llama).parameters
