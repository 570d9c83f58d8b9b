"""Teacher-forced LM scoring without a GPU: the numpy restatement (tests/lm_score_numpy.py over oracle.roformer's functions, causal over
all positions) against the reference's prefix evaluation recorded in tests/golden/lm_score.npz, Roformer.score's argument checks, the C ABI's
new names, get_topk_acc and the tools' argument parsing."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch
import yaml

from conftest import GOLDEN, ROOT

LOGITS_TOL = 2e-5      # the project's LM logits bound; lp / loss: eps = 2 * LOGITS_TOL * absmax (log-sum-exp is 1-Lipschitz in the max norm)


@pytest.fixture(scope="module")
def lm():
    from text2semantic.utils import get_language_model
    return get_language_model(**yaml.safe_load(open(os.path.join(GOLDEN, "config_lm_like_reference.yaml"))))


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_numpy_restatement_vs_reference_prefix_evaluation(golden, lm, tag):
    import lm_score_numpy as N
    s, g = golden("lm_score.npz"), golden("roformer.npz")
    w = {k: v.detach().numpy() for k, v in lm.state_dict().items()}
    enc_len = s["c_enc_len"] if tag == "c" else None
    logits, lp, rank, loss, n = N.score(w, lm.cfg, g["phone"], g["tone"], g["spk_id"], s[tag + "_semantic"], s[tag + "_labels"], s[tag + "_sem_len"], enc_len)
    eps = 2 * LOGITS_TOL * float(s[tag + "_absmax"])
    counted = s[tag + "_rank"] >= 0
    if tag == "a":
        want = g["greedy_logits"].transpose(1, 0, 2)
        assert np.abs(logits[:, : want.shape[1]] - want).max() / np.abs(want).max() < LOGITS_TOL
    if tag == "b":
        assert np.abs(logits[0] - s["b_logits_row0"]).max() / np.abs(s["b_logits_row0"]).max() < LOGITS_TOL
    assert n == int(s[tag + "_n_counted"]) and np.array_equal(rank >= 0, counted)
    assert np.abs(lp - s[tag + "_lp"]).max() < eps and abs(loss - float(s[tag + "_loss"])) < eps
    assert (rank[counted] >= s[tag + "_rank_lo"][counted]).all() and (rank[counted] <= s[tag + "_rank_hi"][counted]).all()
    pinned = counted & (s[tag + "_rank_lo"] == s[tag + "_rank_hi"])
    assert 2 * pinned.sum() >= counted.sum() and np.array_equal(rank[pinned], s[tag + "_rank"][pinned])


def test_fixture_holds_what_the_recipe_states(golden):
    s = golden("lm_score.npz")
    assert s["a_semantic"].shape == (2, 24) and s["b_semantic"].shape == (2, 33) and s["c_semantic"].shape == (2, 33)
    assert (s["a_rank"] == 0).all()                                      # greedy tokens: the top-5 path
    r = s["b_rank"][s["b_rank"] >= 0]
    assert r.min() >= 5 and r.max() > 3000                               # random tokens: ranks spread over the vocabulary
    assert s["c_sem_len"].tolist() == [33, 20] and s["c_enc_len"].tolist() == [23, 15]
    assert (s["c_semantic"][1, 20:] == -100).all() and (s["c_labels"][1, [5, 6, 12]] == -100).all()
    assert (s["c_rank"][1, [4, 5, 11]] == -1).all() and (s["c_rank"][1, 19:] == -1).all() and int(s["c_n_counted"]) == 32 + 19 - 3
    assert os.path.getsize(os.path.join(GOLDEN, "lm_score.npz")) < 700 * 1024


def test_score_argument_checks(lm):
    from text2semantic.roformer.roformer import LMScore, Roformer
    sig = inspect.signature(Roformer.score)
    assert list(sig.parameters)[1:] == ["phone", "tone", "semantic", "attention_mask", "encoder_attention_mask", "labels", "spk_id", "return_logits"]
    assert LMScore._fields == ("loss", "token_logprobs", "ranks", "seq_logprob", "n_tokens", "logits")
    ph, sem = torch.ones(1, 4, dtype=torch.long), torch.ones(1, 6, dtype=torch.long)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lm.score(ph, ph, sem)
    with pytest.raises(NotImplementedError, match="right-padded"):
        lm.score(ph, ph, sem, attention_mask=torch.tensor([[1, 1, 0, 1, 1, 1]]))
    with pytest.raises(NotImplementedError, match="right-padded"):
        lm.score(ph, ph, sem, encoder_attention_mask=torch.tensor([[0, 1, 1, 1]]))
    with pytest.raises(ValueError, match="labels"):
        lm.score(ph, ph, sem, labels=torch.ones(1, 5, dtype=torch.long))
    with pytest.raises(ValueError, match="T"):
        lm.score(ph, ph, sem[:, :1])
    with pytest.raises(ValueError, match="T"):
        lm.score(ph, ph, torch.ones(1, lm.cfg["max_pos"] + 1, dtype=torch.long))
    with pytest.raises(ValueError, match="semantic"):
        lm.score(ph, ph, torch.ones(2, 6, dtype=torch.long))


def test_forward_still_raises_and_points_at_score(lm):
    ph = torch.ones(1, 4, dtype=torch.long)
    with pytest.raises(NotImplementedError, match="score"):
        lm(ph, ph, ph)
    with pytest.raises(NotImplementedError):
        lm.forward(ph, ph, ph, labels=ph)


def test_new_symbols_in_header_and_binding():
    from lds import native
    hdr = open(os.path.join(ROOT, "include", "lds.h")).read()
    for name, kinds in (("lds_lm_score_workspace_bytes", "piiip"), ("lds_lm_score", "pppiipppippppppzp")):
        assert f"int {name}(" in hdr and name in native.EXPORTS and native.SIGNATURES[name] == "i:" + kinds
    decl = hdr[hdr.index("int lds_lm_score("):]
    decl = decl[: decl.index(";")]
    assert decl.count(",") + 1 == len("pppiipppippppppzp")
    if os.path.exists(native.LIB_PATH):
        L = native.lib()
        assert hasattr(L, "lds_lm_score") and hasattr(L, "lds_lm_score_workspace_bytes")
    assert hasattr(native.LM, "score")


def test_get_topk_acc_equals_the_list_comprehension():
    from text2semantic.utils import get_topk_acc
    assert list(inspect.signature(get_topk_acc).parameters) == ["gt_token", "logits", "k"] and inspect.signature(get_topk_acc).parameters["k"].default == 5
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(200, 50, generator=g)
    gt = torch.randint(0, 50, (200,), generator=g)
    for k in (1, 5, 17):
        topk = torch.topk(logits, k, dim=-1).indices.numpy()
        want = sum(1 if gt.numpy()[i] in topk[i] else 0 for i in range(len(gt))) / len(gt)
        assert get_topk_acc(gt, logits, k=k) == pytest.approx(want, abs=1e-7)
        # and the rank form Roformer.score reports: rank < k
        rank = (logits > logits.gather(1, gt[:, None])).sum(1)
        assert float((rank < k).float().mean()) == pytest.approx(want, abs=1e-7)
    assert 0.0 < get_topk_acc(gt, logits) < 1.0


def test_tools_argument_parsing():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import infer_tts
    import validate_lm
    a = validate_lm.parse_args(["--synthetic"])
    assert a.synthetic and a.topk == 5 and a.synthetic_items == 4 and a.out is None
    a = validate_lm.parse_args(["-m", "exp/lm/model_1.pt", "-d", "data/val", "-o", "v.json", "-k", "3"])
    assert (a.model, a.data, a.out, a.topk) == ("exp/lm/model_1.pt", "data/val", "v.json", 3)
    for bad in ([], ["-m", "x.pt"], ["--synthetic", "-k", "0"]):
        with pytest.raises(SystemExit):
            validate_lm.parse_args(bad)
    items = list(validate_lm.synthetic_items(3, 40))
    assert [len(i[3]) for i in items] == [40, 43, 46] and all(len(i[1]) == len(i[2]) for i in items) and max(i[3].max() for i in items) < 4096
    assert infer_tts.parse_args(["--synthetic"]).candidates == 1 and infer_tts.parse_args(["--synthetic", "--candidates", "3"]).candidates == 3
    assert callable(infer_tts.pick_candidate) and callable(infer_tts.text2semantic_candidates)
