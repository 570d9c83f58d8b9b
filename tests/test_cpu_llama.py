"""CPU-side checks of the text2semantic Llama (no GPU): the parameter shapes equal the reference's manifest, the numpy restatement
(tests/llama_numpy.py) reproduces every recorded case of the reference's own generate, the id arithmetic is the reference's, everything that is
not built refuses, `get_language_model` dispatches, and the C ABI declares the entries."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import llama_numpy as LN

LOGITS_TOL = 2e-5      # the project's LM logits bound
MIN_MARGIN = 1e-3


@pytest.fixture(scope="module")
def fx():
    f = dict(np.load(os.path.join(GOLDEN, "llama.npz")))
    f["cases"] = json.loads(bytes(f["cases_json"]).decode())
    f["toy"] = json.loads(bytes(f["toy_json"]).decode())
    return f


def toy_model(fx):
    """(cfg, seeded state) of the fixtures' model"""
    from lds import arch
    toy = dict(fx["toy"])
    cfg = arch.llama_config(semantic_kmeans_num=toy.pop("semantic_kmeans_num"), **toy)
    return cfg, arch.llama_init_state(cfg, int(fx["weight_seed"]))


def case_state(fx, state, cfg, tag):
    if tag != "eos":
        return state
    st = dict(state)
    st["llama.lm_head.weight"] = state["llama.lm_head.weight"].copy()
    st["llama.lm_head.weight"][cfg["eos"]] = fx["eos_row"]
    return st


def test_param_shapes_match_reference_manifest(fx):
    from lds import arch
    cfg, _ = toy_model(fx)
    manifest = json.load(open(os.path.join(GOLDEN, "manifest_llama.json")))
    shapes = arch.llama_param_shapes(cfg)
    assert {k: list(v) for k, v in shapes.items()} == manifest
    assert list(shapes) == list(manifest)      # the reference's key order as well
    assert cfg["vocab"] == 172 and cfg["vocab"] % 64 and cfg["heads"] // cfg["kv_heads"] == 3 and cfg["head_dim"] == 16


def test_module_keys_ids_and_inverse_frequencies(fx):
    """the module carries the reference's state-dict keys and attribute names; its rotary inverse frequencies are the reference model's, bit for bit"""
    import torch
    from lds import arch
    from text2semantic.llama.llama import Llama
    toy = dict(fx["toy"])
    K = toy.pop("semantic_kmeans_num")
    config = dict(toy)
    m = Llama(config, semantic_kmeans_num=K, codebook_path="/nonexistent")
    assert list(m.state_dict()) == list(json.load(open(os.path.join(GOLDEN, "manifest_llama.json"))))
    assert np.array_equal(m.inv_freq.numpy(), fx["inv_freq"])
    # llama.py:36-61: the phone-side ids, the shift, and the ids written into the caller's config
    assert (m.BOS, m.EOS, m.PAD, m.semantic_token_shift, m.num_tones) == (108, 109, 110, 108, arch.NUM_TONES)
    assert (m.config.bos_token_id, m.config.eos_token_id, m.config.pad_token_id, m.config.vocab_size) == (108 + K, 108 + K + 1, 108 + K + 2, 108 + K + 3)
    assert config["vocab_size"] == 108 + K + 3      # (the reference mutates the config it is given)
    # the collision the reference's numbering has: phone BOS / EOS / PAD are the shifted semantic ids 0, 1, 2
    assert (m.BOS - m.semantic_token_shift, m.EOS - m.semantic_token_shift, m.PAD - m.semantic_token_shift) == (0, 1, 2)
    ids, lens = m.input_ids(torch.tensor([[5, 6, 7, 0], [9, 0, 0, 0]]), torch.tensor([[1, 1, 1, 0], [1, 0, 0, 0]]))
    pad = 108 + K + 2
    assert ids.tolist() == [[108, 5, 6, 7, 109, 108 + K, pad], [108, 9, 109, 108 + K, pad, pad, pad]] and lens == [6, 4]
    ids, lens = m.input_ids(torch.tensor([[5, 6, 7]]))
    assert ids.tolist() == [[108, 5, 6, 7, 109, 108 + K]] and lens == [6]      # llama.py:148-152
    # an HF-style namespace works like a dict; transformers is never imported by the module
    import types
    ns = types.SimpleNamespace(**toy, rope_parameters={"rope_type": "default", "rope_theta": 10000.0})
    m2 = Llama(ns, semantic_kmeans_num=K, codebook_path="/nonexistent")
    assert ns.vocab_size == 108 + K + 3 and m2.cfg == m.cfg
    import subprocess
    import sys
    code = "import sys; sys.path[:0] = [%r, %r]; import text2semantic.llama.llama; assert 'transformers' not in sys.modules" % (
        os.path.join(ROOT, "latent-diffusion-speech_amd"), ROOT)
    subprocess.run([sys.executable, "-c", code], check=True)


def test_codebook_seeding_is_off_by_one_like_the_reference(tmp_path, fx):
    """llama.py:66-71 writes the centres to the rows len(symbols) - 1 ..: one below the first semantic id"""
    import torch
    from text2semantic.llama.llama import Llama
    toy = dict(fx["toy"])
    K = toy.pop("semantic_kmeans_num")
    centers = np.arange(K * toy["hidden_size"], dtype=np.float32).reshape(K, toy["hidden_size"])
    path = tmp_path / "codebook.pt"
    torch.save({"n_features_in_": toy["hidden_size"], "_n_threads": 1, "cluster_centers_": centers}, path)      # cluster.get_cluster_model's format
    m = Llama(dict(toy), semantic_kmeans_num=K, codebook_path=str(path))
    emb = m.llama.model.embed_tokens.weight.detach().numpy()
    assert np.array_equal(emb[107:107 + K], centers)
    plain = Llama(dict(toy), semantic_kmeans_num=K, codebook_path="/nonexistent").llama.model.embed_tokens.weight.detach().numpy()
    assert np.array_equal(emb[:107], plain[:107]) and np.array_equal(emb[107 + K:], plain[107 + K:])


@pytest.mark.parametrize("tag", ["greedy", "sample", "eos", "penalty"])
def test_restatement_reproduces_the_reference(fx, tag):
    cfg, state = toy_model(fx)
    st = case_state(fx, state, cfg, tag)
    kw = dict(fx["cases"][tag])
    max_length = kw.pop("max_length")
    for b in range(2):
        p = f"{tag}_r{b}_"
        assert float(fx[p + "margin"]) >= MIN_MARGIN      # the recorded run rests on no near-tie: exact tokens may be demanded
        ids = LN.prompt_ids(cfg, fx[f"phone_r{b}"])
        seq, logits, margins = LN.generate_row(st, cfg, fx["inv_freq"], ids, max_length, uniforms=fx.get(p + "uniforms"), **kw)
        ref = fx[p + "logits"]
        relmax = np.abs(logits[:len(ref)] - ref).max() / np.abs(ref).max()
        print(f"{tag} r{b}: logits relmax {relmax:.3e}, restated margin {margins.min():.3e}")
        assert margins.min() >= MIN_MARGIN / 2
        assert relmax < LOGITS_TOL
        assert np.array_equal(seq[len(ids):] - cfg["shift"], fx[p + "tokens"])
    if tag == "eos":
        ends = [len(fx[f"eos_r{b}_tokens"]) for b in range(2)]
        assert ends[0] != ends[1] and all(fx[f"eos_r{b}_tokens"][-1] == cfg["eos"] - cfg["shift"] for b in range(2))


def test_penalty_hits_semantic_tokens_0_and_1_from_the_first_step(fx):
    """ids 108 and 109 (phone BOS / EOS) are in every prompt and ARE the shifted semantic ids 0 and 1: HF's repetition penalty, which sees
    the whole input_ids, penalises those two from the first step; the prompt's n-grams count for the ban"""
    cfg, _ = toy_model(fx)
    lg = np.linspace(-1.0, 1.0, cfg["vocab"] - cfg["shift"]).astype(np.float32)
    lg[0], lg[1] = 3.0, 2.5
    hist = [t - cfg["shift"] for t in LN.prompt_ids(cfg, [5, 6, 7])]
    assert hist[0] == 0 and hist[-2] == 1 and hist[1] < 0
    assert LN.choose(lg, hist)[0] == 0
    tok, _ = LN.choose(lg, hist, repetition_penalty=4.0)
    assert tok == len(lg) - 1      # 3.0 / 4 and 2.5 / 4 fall below the ramp's top
    # the history ends ... 7, 9, 7: the bigram (7, 9) bans 9; the shifted phone ids are negative, never candidates
    h2 = hist + [7, 9, 7]
    assert LN.choose(np.where(np.arange(len(lg)) == 9, 5.0, lg).astype(np.float32), h2, no_repeat_ngram_size=2)[0] != 9


def test_refusals(fx):
    import torch
    from text2semantic.llama.llama import Llama
    toy = dict(fx["toy"])
    K = toy.pop("semantic_kmeans_num")
    with pytest.raises(NotImplementedError, match="text"):
        Llama(dict(toy), mode="text", semantic_kmeans_num=K)
    for bad in (dict(attention_bias=True), dict(mlp_bias=True)):
        with pytest.raises(NotImplementedError, match="bias"):
            Llama(dict(toy, **bad), semantic_kmeans_num=K)
    with pytest.raises(NotImplementedError, match="rope"):
        Llama(dict(toy, rope_parameters={"rope_type": "llama3", "rope_theta": 10000.0}), semantic_kmeans_num=K)
    with pytest.raises(NotImplementedError, match="rope"):
        Llama(dict(toy, rope_scaling={"type": "linear", "factor": 2.0}), semantic_kmeans_num=K)
    with pytest.raises(NotImplementedError, match="silu"):
        Llama(dict(toy, hidden_act="gelu"), semantic_kmeans_num=K)
    m = Llama(dict(toy), semantic_kmeans_num=K, codebook_path="/nonexistent")
    ph = torch.tensor([[1, 2, 3]])
    with pytest.raises(NotImplementedError, match="end gate"):
        m.generate(ph, ph, end_gate_threshold=0.9)
    with pytest.raises(NotImplementedError, match="beam"):
        m.generate(ph, ph, num_beams=2, max_length=16)
    with pytest.raises(NotImplementedError, match="training"):
        m(ph, ph, ph)
    with pytest.raises(ValueError, match="max_length"):
        m.generate(ph, ph, max_length=6)      # the prompt alone has 6 ids
    with pytest.raises(ValueError, match="max_position_embeddings"):
        m.generate(ph, ph, max_length=129)
    with pytest.raises(NotImplementedError, match="right-padded"):
        m.generate(torch.tensor([[1, 2, 3]]), ph, attention_mask=torch.tensor([[0, 1, 1]]), max_length=16)
    with pytest.raises(RuntimeError, match="HIP device"):
        m.generate(ph, ph, max_length=16)      # no CPU fallback


def test_get_language_model_dispatch(fx):
    from text2semantic.llama.llama import Llama
    from text2semantic.utils import get_language_model
    toy = dict(fx["toy"])
    K = toy.pop("semantic_kmeans_num")
    args = {"common": {"n_spk": 1},
            "text2semantic": {"model": {"type": "llama", "mode": "phone", "semantic_kmeans_num": K, "codebook_path": "/nonexistent", "llama": toy},
                              "train": {"use_flash_attn": False}}}
    m = get_language_model(**args)
    assert isinstance(m, Llama) and m.cfg["vocab"] == 108 + K + 3 and m.cfg["kv_heads"] == 2
    for other in ("gpt", "Llama", ""):
        args["text2semantic"]["model"]["type"] = other
        with pytest.raises(ValueError, match="Unknown Model"):
            get_language_model(**args)


def test_abi_entries_declared():
    from lds import native
    hdr = open(os.path.join(ROOT, "include", "lds.h")).read()
    for fn in ("lds_llama_create", "lds_llama_destroy", "lds_llama_workspace_bytes", "lds_llama_generate"):
        assert fn in native.EXPORTS and fn + "(" in hdr
    assert native.SIGNATURES["lds_llama_generate"] == "i:pppiiippppppzp"
    assert [f[0] for f in native.LlamaCfg._fields_] == ["hidden", "heads", "kv_heads", "head_dim", "inter", "layers", "vocab", "max_pos", "eps", "rope_theta",
                                                        "first_free_id", "bos", "eos", "pad"]
    assert "llama.py:" in hdr      # the entries cite the reference lines they replace


def test_create_refuses_unsupported_shapes_before_any_device_call():
    """the shape checks of lds_llama_create come before anything touches a device: they answer on a machine without one"""
    import ctypes as ct
    from lds import native
    L = native.lib()
    base = dict(hidden=96, heads=6, kv_heads=2, head_dim=16, inter=160, layers=2, vocab=172, max_pos=128, eps=1e-6, rope_theta=10000.0, first_free_id=108,
                bos=169, eos=170, pad=171)
    for bad, word in ((dict(head_dim=24), b"head_dim"), (dict(head_dim=272), b"head_dim"), (dict(head_dim=8), b"head_dim"), (dict(kv_heads=4), b"divide"),
                      (dict(vocab=108 + 8193, bos=200, eos=201, pad=202), b"columns"), (dict(hidden=4096), b"hidden"), (dict(eos=107), b"eos")):
        c = native.LlamaCfg(**dict(base, **bad))
        h = ct.c_void_p()
        empty = (ct.c_void_p * 1)()
        assert L.lds_llama_create(ct.byref(c), 0, empty, empty, empty, ct.byref(h)) == -1 and word in L.lds_last_error() and not h.value
    o = native.LMDecodeOpts(0, 5, 1.0, 1.0, 1.0, 0, 2, 1)
    n = ct.c_int(-5)
    assert L.lds_llama_generate(None, None, None, 1, 4, 16, ct.byref(o), None, None, None, ct.byref(n), None, 0, None) == -1 and b"beam" in L.lds_last_error()
    assert n.value == -5
