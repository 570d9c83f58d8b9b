"""Prompted LM generation without a GPU: the numpy restatement (tests/lm_prompt_numpy.py over oracle.roformer's functions, every row alone)
against the reference's HF call started from input_ids= (tests/golden/lm_prompt.npz), what the fixture holds, Roformer.generate's prompt
checks, the C ABI's new names and the argument checks of the C entry that need no device."""
import ctypes as C
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch
import yaml

from conftest import GOLDEN, ROOT

LOGITS_TOL = 2e-5      # the project's LM logits bound
CASES = ["greedy", "sample", "ngram", "penalty", "eos", "ragged_greedy", "ragged_sample"]


@pytest.fixture(scope="module")
def lm():
    from text2semantic.utils import get_language_model
    return get_language_model(**yaml.safe_load(open(os.path.join(GOLDEN, "config_lm_like_reference.yaml"))))


@pytest.mark.parametrize("tag", CASES)
def test_numpy_restatement_vs_reference(golden, lm, tag):
    import lm_prompt_numpy as N
    fx, g = golden("lm_prompt.npz"), golden("roformer.npz")
    kw = json.loads(bytes(fx["cases_json"]).decode())[tag]
    w = {k: v.detach().numpy().copy() for k, v in lm.state_dict().items()}
    if tag == "eos":
        w["semantic_decoder.cls.predictions.decoder.bias"][lm.cfg["sem_eos"]] += fx["eos_bias"]
    ragged = tag.startswith("ragged")
    toks, logits = N.generate(w, lm.cfg, g["phone"], g["tone"], g["spk_id"], fx[tag + "_prompt"], fx[tag + "_prompt_len"], enc_len=fx["ragged_len"] if ragged else None,
                              uniforms=fx[tag + "_uniforms"] if kw.get("do_sample") else None, **kw)
    want = fx[tag + "_tokens"]
    assert toks.shape == want.shape and np.array_equal(toks, want), (toks.tolist(), want.tolist())
    if tag == "greedy":
        ref = fx["greedy_logits_row0"]
        assert logits[0].shape == ref.shape and np.abs(logits[0] - ref).max() / np.abs(ref).max() < LOGITS_TOL


def test_fixture_holds_what_the_recipe_states(golden):
    fx, g = golden("lm_prompt.npz"), golden("roformer.npz")
    cases = json.loads(bytes(fx["cases_json"]).decode())
    assert sorted(cases) == sorted(CASES)
    bos, eos, pad = 4096, 4097, 4098
    for tag in CASES:
        p, n, t = fx[tag + "_prompt"], fx[tag + "_prompt_len"], fx[tag + "_tokens"]
        assert float(fx[tag + "_margin"]) >= 1e-3 and p.shape[0] == 2 and (p[:, 0] == bos).all() and t.shape[1] <= cases[tag]["max_length"]
        for b in range(2):
            assert np.array_equal(t[b, : n[b]], p[b, : n[b]]) and (p[b, 1: n[b]] < 4096).all()
        assert (tag + "_uniforms" in fx) == bool(cases[tag].get("do_sample"))
    assert fx["greedy_prompt_len"].tolist() == [9, 9] and fx["greedy_tokens"].shape == (2, 24) and fx["greedy_logits_row0"].shape == (15, 4099)
    assert fx["sample_tokens"].shape == (2, 40) and cases["sample"]["top_k"] == 5 and cases["sample"]["repetition_penalty"] == 1.2
    # n-gram and penalty: prompts cut from the unprompted greedy run; in the looping row the plain continuation would repeat the loop's token
    for tag in ("ngram", "penalty"):
        assert np.array_equal(fx[tag + "_prompt"], g["greedy_tokens"][:, :16])
        assert fx[tag + "_tokens"][1, 16] != g["greedy_tokens"][1, 16] and g["greedy_tokens"][1, 16] in fx[tag + "_prompt"][1]
    assert (int(fx["ngram_prompt"][1, 15]), int(g["greedy_tokens"][1, 16])) in set(zip(fx["ngram_prompt"][1, :-1].tolist(), fx["ngram_prompt"][1, 1:].tolist()))
    assert fx["ragged_sample_prompt_len"].tolist() == [9, 4] and fx["ragged_greedy_prompt_len"].tolist() == [9, 4] and fx["ragged_len"].tolist() == [23, 15]
    e = fx["eos_tokens"]
    ends = [int(np.argmax(r == eos)) if (r == eos).any() else None for r in e]
    assert e.shape[1] == 40 and sorted(ends, key=str) == sorted([None, min(x for x in ends if x is not None)], key=str)
    x = [x for x in ends if x is not None][0]
    assert 9 <= x < 14 and (e[ends.index(x), x + 1:] == pad).all()
    assert os.path.getsize(os.path.join(GOLDEN, "lm_prompt.npz")) < 400 * 1024


def test_generate_prompt_argument_checks(lm):
    from text2semantic.roformer.roformer import Roformer
    names = list(inspect.signature(Roformer.generate).parameters)
    assert "semantic_prompt" in names and "prompt_attention_mask" in names and names.index("semantic_prompt") > names.index("return_logits")
    bos = lm.semantic_bos_token_id
    ph = torch.ones(2, 4, dtype=torch.long)
    ok = torch.tensor([[bos, 5, 6, 7], [bos, 8, 9, 10]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # a valid prompt passes every check; then the device is missing
        lm.generate(ph, ph, max_length=8, semantic_prompt=ok)
    with pytest.raises(ValueError, match="BOS"):
        lm.generate(ph, ph, max_length=8, semantic_prompt=torch.tensor([[bos, 5, 6, 7], [3, 8, 9, 10]]))
    with pytest.raises(ValueError, match="row 1.*must lie in"):
        lm.generate(ph, ph, max_length=8, semantic_prompt=torch.tensor([[bos, 5, 6, 7], [bos, 8, 4096, 10]]))
    with pytest.raises(ValueError, match="must lie in"):
        lm.generate(ph, ph, max_length=8, semantic_prompt=torch.tensor([[bos, 5, 6, 7], [bos, -1, 9, 10]]))
    # the same id beyond the row's length is never looked at
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lm.generate(ph, ph, max_length=8, semantic_prompt=torch.tensor([[bos, 5, 6, 7], [bos, 8, 10 ** 9, -5]]), prompt_attention_mask=torch.tensor([[1, 1, 1, 1], [1, 1, 0, 0]]))
    with pytest.raises(ValueError, match="row 0.*max_length"):
        lm.generate(ph, ph, max_length=4, semantic_prompt=ok)
    with pytest.raises(ValueError, match="row 0.*max_length"):
        lm.generate(ph, ph, max_length=3, semantic_prompt=ok, prompt_attention_mask=torch.tensor([[1, 1, 1, 0], [1, 1, 0, 0]]))
    with pytest.raises(NotImplementedError, match="right-padded"):
        lm.generate(ph, ph, max_length=8, semantic_prompt=ok, prompt_attention_mask=torch.tensor([[1, 1, 1, 1], [0, 1, 1, 1]]))
    with pytest.raises(NotImplementedError, match="right-padded"):
        lm.generate(ph, ph, max_length=8, semantic_prompt=ok, prompt_attention_mask=torch.tensor([[1, 1, 1, 1], [1, 0, 1, 0]]))
    with pytest.raises(NotImplementedError, match="beam search from a prompt"):
        lm.generate(ph, ph, max_length=8, do_sample=False, num_beams=2, semantic_prompt=ok)
    with pytest.raises(ValueError, match="semantic_prompt"):
        lm.generate(ph, ph, max_length=8, semantic_prompt=ok[:1])
    with pytest.raises(ValueError, match="prompt_attention_mask"):
        lm.generate(ph, ph, max_length=8, semantic_prompt=ok, prompt_attention_mask=torch.ones(2, 3, dtype=torch.long))
    with pytest.raises(ValueError, match="needs semantic_prompt"):
        lm.generate(ph, ph, max_length=8, prompt_attention_mask=torch.ones(2, 4, dtype=torch.long))


def test_new_symbols_in_header_and_binding():
    from lds import native
    hdr = open(os.path.join(ROOT, "include", "lds.h")).read()
    for name, kinds in (("lds_lm_workspace_bytes_prompt", "piiiip"), ("lds_lm_generate_prompt", "pppiiipppipppppzp")):
        assert f"int {name}(" in hdr and name in native.EXPORTS and native.SIGNATURES[name] == "i:" + kinds
        decl = hdr[hdr.index(f"int {name}("):]
        assert decl[: decl.index(";")].count(",") + 1 == len(kinds)
    assert "roformer.py:235-242" in hdr and "input_ids" in hdr
    if os.path.exists(native.LIB_PATH):
        L = native.lib()
        assert hasattr(L, "lds_lm_generate_prompt") and hasattr(L, "lds_lm_workspace_bytes_prompt")
    assert hasattr(native.LM, "generate_prompt")


def test_entry_argument_checks_without_a_device():
    """the checks that need no model come first and give LDS_EINVAL before anything touches the device"""
    from lds import native
    L = native.lib()
    nb = C.c_size_t()
    assert L.lds_lm_workspace_bytes_prompt(None, 65, 23, 40, 9, C.byref(nb)) == -1 and "at most 64" in L.lds_last_error().decode()
    assert L.lds_lm_workspace_bytes_prompt(None, 2, 23, 40, 0, C.byref(nb)) == -1
    assert L.lds_lm_workspace_bytes_prompt(None, 2, 23, 40, 9, C.byref(nb)) == -1 and "bad argument" in L.lds_last_error().decode()
    dummy = (C.c_float * 8)()
    toks, n = (C.c_int64 * 80)(), C.c_int()
    prompt = (C.c_int64 * (65 * 9))()
    wsb = (C.c_char * 64)()

    def gen(plen, B=2, max_length=40, P=9, **kw):
        o = native.LMDecodeOpts(0, 5, 1.0, 1.0, 1.0, 0, 1, 1)
        for k, v in kw.items():
            setattr(o, k, v)
        pl = None if plen is None else C.cast((C.c_int32 * B)(*plen), C.c_void_p)
        return L.lds_lm_generate_prompt(None, dummy, None, B, 23, max_length, C.byref(o), prompt, pl, P, None, toks, None, C.byref(n), wsb, C.c_size_t(64), None)
    for args, kw, msg in (((([9, 9]),), dict(num_beams=2), "beam search from a prompt"), (([9, 9],), dict(num_beams=9), "num_beams"),
                          (([9, 9],), dict(no_repeat_ngram_size=-1), "no_repeat_ngram_size"), (([9] * 65, 65), {}, "at most 64"),
                          (([9, 0],), {}, "prompt_len[1] = 0 out of range"), (([10, 9],), {}, "prompt_len[0] = 10 out of range"),
                          (([9, 5], 2, 9), {}, "prompt_len[0] = 9 leaves no room below max_length = 9"), ((None, 2, 9), {}, "max_length"),
                          (([9, 9], 2, 40, 0), {}, "bad argument")):
        assert gen(*args, **kw) == -1 and msg in L.lds_last_error().decode(), (args, kw, L.lds_last_error())
    assert gen([9, 4]) == -1 and "bad argument" in L.lds_last_error().decode()      # valid shapes: the missing model is what is refused


def test_tools_argument_parsing():
    sys.path.insert(0, ROOT)
    import infer_tts
    a = infer_tts.parse_args(["--synthetic"])
    assert a.prompt_tokens is None and a.prompt_phones is None and a.prompt_audio is None and not a.keep_prompt
    a = infer_tts.parse_args(["--synthetic", "--prompt_tokens", "t.npy", "--prompt_phones", "p.npy", "--keep_prompt"])
    assert (a.prompt_tokens, a.prompt_phones, a.keep_prompt) == ("t.npy", "p.npy", True)
    assert "prompt_rows" in inspect.signature(infer_tts.text2semantic_rows).parameters
    assert inspect.signature(infer_tts.pick_candidate).parameters["prompt_len"].default == 1
