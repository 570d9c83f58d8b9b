"""Generate the Whisper text decoder's golden fixtures from the reference's own blocks.

Runs ONLY in the build container (needs /root/reference); the GPU box never sees the reference.  Writes (default: next to this script,
`--out DIR` elsewhere) whisper_decoder.npz and manifest_whisper_decoder.json.

The oracle.  The reference carries the decoder's blocks (encoder/whisper/model.py:42-110: MultiHeadAttention, ResidualAttentionBlock(
cross_attention=True)) and its interface (Whisper.logits / Whisper.forward) but builds no `self.decoder`.  OpenAI's TextDecoder is composed
here, in this recipe's own text, from those blocks: token embedding + learned positions, the blocks under the triu(-inf) mask, `ln`,
x @ token_embedding.weight.T.  It is evaluated in float64; two lines of the reference fall back to float32 whatever the module's dtype --
LayerNorm.forward's `x.float()` (model.py:25) and qkv_attention's `qk = qk.float()` (model.py:80).  For a float64 evaluation the first runs
nn.LayerNorm.forward and the second runs with torch.Tensor.float as the identity inside that one call (with only LayerNorm replaced, as make_whisper_fixtures.py does for the encoder, two "float64"
implementations still differ by 1e-7 x absmax: the softmax input has been rounded to float32).  Every row of a ragged batch is evaluated
alone on its own n_frames[b] frames.

The cross-check.  transformers' WhisperForConditionalGeneration with the same weights under HF's names (query / key / value / out ->
q_proj / k_proj / v_proj / out_proj, attn / cross_attn -> self_attn / encoder_attn, mlp.0 / mlp.2 -> fc1 / fc2, *_ln -> *_layer_norm,
proj_out tied) in float64 gives the same logits (the agreement reached is printed and stored as `hf_logits_*`) and, through
generate(encoder_outputs=..., decoder_input_ids=...) with the suppress lists passed explicitly, the same greedy ids (asserted).  Skipped with
a message when the package is absent; `hf_*` then hold -1.

Stored per configuration X (tests/whisper_decoder_numpy.py CONFIGS: A, B, C; inputs from its `inputs`, weights from lds/arch.py
whisper_decoder_init_state -- results only, no inputs):
  logits_X [3][9][V] float64      teacher-forced, n_frames (1, 37, 100), tok_len (9, 5, 2) (ids at and beyond count as 0)
  gen_tokens_X [3][cap] int64, gen_len_X [3], gen_lp_X [3][max_new] float64      the greedy paths from prompts of (1, 2, 4) ids, suppress lists on
  gap_X        the oracle's own fp32-against-fp64 error over absmax (logits)
  margin_X     the smallest top-2 logit gap over absmax along the greedy paths; the recipe asserts margin_X >= 1e-3 (50 x the 2e-5 logits
               bound of the GPU tests) and otherwise takes the next seed; seed_X is the one used
  A also: logits_A1500 / gen_*_A1500, one row on 1500 frames.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_whisper_decoder_fixtures.py [--out DIR]
    python tests/golden/make_whisper_decoder_fixtures.py --check      # regenerate into a temporary directory, compare bit for bit
"""
import argparse
import importlib.util
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PKG = os.path.join(ROOT, "latent-diffusion-speech_amd")
REF = "/root/reference"
FILES = ("manifest_whisper_decoder.json", "whisper_decoder.npz")
MARGIN_MIN = 1e-3
sys.dont_write_bytecode = True


def _load_by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def check():
    with tempfile.TemporaryDirectory() as out_dir:
        env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
        env.pop("PYTHONPATH", None)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--out", out_dir], env=env, cwd=out_dir, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            print(r.stdout[-4000:])
            return 1
        bad = []
        for f in FILES:
            a, b = os.path.join(HERE, f), os.path.join(out_dir, f)
            if f.endswith(".json"):
                if json.load(open(a)) != json.load(open(b)):
                    bad.append(f)
                continue
            za, zb = np.load(a), np.load(b)
            if sorted(za.files) != sorted(zb.files):
                bad.append(f)
                continue
            for k in za.files:
                x, y = za[k], zb[k]
                if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
                    bad.append(f"{f}:{k}")
        print("whisper decoder fixtures", "differ: " + ", ".join(bad) if bad else "reproduce bit for bit")
        return 1 if bad else 0


def main(out):
    arch = _load_by_path("_amd_arch", os.path.join(PKG, "lds", "arch.py"))
    init_weights = _load_by_path("_amd_init_weights", os.path.join(PKG, "lds", "init_weights.py"))
    dnp = _load_by_path("_amd_whisper_decoder_numpy", os.path.join(ROOT, "tests", "whisper_decoder_numpy.py"))
    sys.path[:] = [p for p in sys.path if os.path.realpath(p or ".") not in (os.path.realpath(PKG), os.path.realpath(ROOT), os.path.realpath(HERE))]
    sys.path.insert(0, REF)
    import torch
    from torch import nn
    torch.set_grad_enabled(False)
    torch.set_num_threads(8)
    from encoder.whisper import model as ref_model
    assert os.path.realpath(ref_model.__file__).startswith(REF + os.sep)

    class TextDecoder(nn.Module):
        """OpenAI's TextDecoder over the reference's blocks"""
        def __init__(self, n_vocab, n_ctx, n_state, n_head, n_layer):
            super().__init__()
            self.token_embedding = nn.Embedding(n_vocab, n_state)
            self.positional_embedding = nn.Parameter(torch.empty(n_ctx, n_state))
            self.blocks = nn.ModuleList([ref_model.ResidualAttentionBlock(n_state, n_head, cross_attention=True) for _ in range(n_layer)])
            self.ln = ref_model.LayerNorm(n_state)
            self.register_buffer("mask", torch.empty(n_ctx, n_ctx).fill_(-np.inf).triu_(1), persistent=False)

        def forward(self, x, xa):
            x = self.token_embedding(x) + self.positional_embedding[: x.shape[-1]]
            x = x.to(xa.dtype)
            for block in self.blocks:
                x = block(x, xa, mask=self.mask)
            x = self.ln(x)
            return x @ torch.transpose(self.token_embedding.weight.to(x.dtype), 0, 1)

    class in_double:
        """A float64 evaluation of the reference's blocks.  model.py:25 (LayerNorm.forward: `x.float()`) runs the parent's forward instead, as in
        make_whisper_fixtures.py; model.py:80 (`qk = qk.float()` inside qkv_attention) is the reference's own function run with Tensor.float as
        the identity for the duration of THAT call only -- nothing else in the process sees the patch."""
        def __enter__(self):
            self.ln, self.qkv = ref_model.LayerNorm.forward, ref_model.MultiHeadAttention.qkv_attention
            real_qkv = self.qkv

            def qkv_in_dtype(mod, q, k, v, mask=None):
                real_float = torch.Tensor.float
                torch.Tensor.float = lambda t: t
                try:
                    return real_qkv(mod, q, k, v, mask)
                finally:
                    torch.Tensor.float = real_float
            ref_model.LayerNorm.forward = nn.LayerNorm.forward
            ref_model.MultiHeadAttention.qkv_attention = qkv_in_dtype

        def __exit__(self, *a):
            ref_model.LayerNorm.forward, ref_model.MultiHeadAttention.qkv_attention = self.ln, self.qkv

    def tt(a):
        return torch.from_numpy(np.ascontiguousarray(a))

    def hf_model(c, state, eos):
        try:
            from transformers import WhisperConfig, WhisperForConditionalGeneration
        except Exception as e:      # the package is optional
            print("transformers is absent, cross-check skipped:", e)
            return None
        C = c["n_state"]
        cfg = WhisperConfig(vocab_size=c["n_vocab"], num_mel_bins=80, encoder_layers=1, encoder_attention_heads=c["n_head"], decoder_layers=c["n_layer"],
                            decoder_attention_heads=c["n_head"], decoder_ffn_dim=4 * C, encoder_ffn_dim=4 * C, d_model=C, max_source_positions=1500,
                            max_target_positions=c["n_text_ctx"], pad_token_id=eos, bos_token_id=eos, eos_token_id=eos, decoder_start_token_id=0,
                            suppress_tokens=None, begin_suppress_tokens=None, activation_function="gelu", scale_embedding=False, dropout=0.0,
                            attention_dropout=0.0, activation_dropout=0.0, tie_word_embeddings=True)
        m = WhisperForConditionalGeneration(cfg).double().eval()
        sd = {}
        for k, v in state.items():
            k = k[len("decoder."):]
            if k == "token_embedding.weight":
                n = "embed_tokens.weight"
            elif k == "positional_embedding":
                n = "embed_positions.weight"
            elif k.startswith("ln."):
                n = "layer_norm." + k[3:]
            else:
                n = k.replace("blocks.", "layers.")
                n = n.replace(".cross_attn_ln.", ".encoder_attn_layer_norm.").replace(".attn_ln.", ".self_attn_layer_norm.").replace(".mlp_ln.", ".final_layer_norm.")
                n = n.replace(".mlp.0.", ".fc1.").replace(".mlp.2.", ".fc2.")
                n = n.replace(".cross_attn.", ".encoder_attn.").replace(".attn.", ".self_attn.")
                n = n.replace(".query.", ".q_proj.").replace(".key.", ".k_proj.").replace(".value.", ".v_proj.").replace(".out.", ".out_proj.")
            sd["model.decoder." + n] = tt(v).double()
        missing, unexpected = m.load_state_dict(sd, strict=False)
        bad = [k for k in missing if k.startswith("model.decoder.") and "k_proj.bias" not in k] + list(unexpected)
        assert not bad, bad
        m.tie_weights()
        assert m.proj_out.weight.data_ptr() == m.model.decoder.embed_tokens.weight.data_ptr() or torch.equal(m.proj_out.weight, m.model.decoder.embed_tokens.weight)
        return m

    res, manifest = {}, {}

    def shapes(n_vocab, n_ctx, n_state, n_head, n_layer):
        with torch.device("meta"):
            d = TextDecoder(n_vocab, n_ctx, n_state, n_head, n_layer)
        return {"decoder." + k: list(v.shape) for k, v in d.state_dict().items()}
    L3 = arch.WHISPER_LARGE_V3_DIMS
    manifest["large_v3"] = shapes(L3["n_vocab"], L3["n_text_ctx"], L3["n_text_state"], L3["n_text_head"], L3["n_text_layer"])

    for name, c in dnp.CONFIGS.items():
        manifest[name] = shapes(c["n_vocab"], c["n_text_ctx"], c["n_state"], c["n_head"], c["n_layer"])
        for seed in range(16):
            state = arch.whisper_decoder_init_state(c["n_vocab"], c["n_text_ctx"], c["n_state"], c["n_layer"], seed, init_weights)
            assert {k: list(v.shape) for k, v in state.items()} == manifest[name]
            inp = dnp.inputs(name, init_weights.uniform, seed)
            dec = TextDecoder(c["n_vocab"], c["n_text_ctx"], c["n_state"], c["n_head"], c["n_layer"]).eval()
            dec.load_state_dict({k[len("decoder."):]: tt(v) for k, v in state.items()})
            dec64 = TextDecoder(c["n_vocab"], c["n_text_ctx"], c["n_state"], c["n_head"], c["n_layer"]).double().eval()
            dec64.load_state_dict({k[len("decoder."):]: tt(v).double() for k, v in state.items()})

            def fwd64(toks, xa):
                with in_double():
                    return dec64(torch.as_tensor(toks, dtype=torch.int64)[None], tt(xa).double()[None])[0].numpy()

            def case(units, n_frames, tok_len, prompts):
                tf = inp["tf_tokens"][: len(n_frames)].copy()
                for b in range(len(n_frames)):
                    tf[b, tok_len[b]:] = 0
                l64 = np.stack([fwd64(tf[b], units[b, : n_frames[b]]) for b in range(len(n_frames))])
                l32 = np.stack([dec(tt(tf[b])[None], tt(units[b, : n_frames[b]])[None])[0].numpy() for b in range(len(n_frames))])
                gap = float(np.abs(l32 - l64).max() / np.abs(l64).max())
                gens = [dnp.greedy_row(None, c, None, prompts[b], c["max_new"], inp["eos"], inp["suppress"], inp["begin_suppress"],
                                       forward=lambda t, b=b: fwd64(t, units[b, : n_frames[b]])) for b in range(len(n_frames))]
                return l64, gap, gens
            l64, gap, gens = case(inp["units"], dnp.N_FRAMES, dnp.TF_LEN, inp["prompts"])
            margin = min(g[3] for g in gens)
            extra = None
            if name == "A":
                extra = case(inp["units_long"], (dnp.T_LONG,), (dnp.TF_S,), inp["prompts"][2:3])
                margin = min(margin, extra[2][0][3])
            print(f"{name} seed {seed}: logits absmax {np.abs(l64).max():.2f} gap {gap:.2e} margin {margin:.2e} lens {[len(g[0]) for g in gens]}")
            if margin >= MARGIN_MIN:
                break
        else:
            raise SystemExit(f"{name}: no seed below 16 gives greedy paths with a top-2 gap of {MARGIN_MIN} x absmax")
        assert margin >= MARGIN_MIN

        def store(tag, l64, gap, gens):
            cap = min(c["n_text_ctx"], max(len(g[0]) for g in gens))
            res[f"logits_{tag}"] = l64
            res[f"gap_{tag}"] = np.float64(gap)
            res[f"gen_tokens_{tag}"] = dnp.pad_rows([g[0] for g in gens], cap, int(inp["eos"]))
            res[f"gen_len_{tag}"] = np.array([len(g[0]) for g in gens], dtype=np.int64)
            res[f"gen_lp_{tag}"] = dnp.pad_rows([g[1] for g in gens], c["max_new"], 0.0)
            res[f"gen_absmax_{tag}"] = np.float64(max(np.abs(g[2]).max() for g in gens))
        store(name, l64, gap, gens)
        if extra:
            store(name + "1500", *extra)
        res[f"margin_{name}"] = np.float64(margin)
        res[f"seed_{name}"] = np.int64(seed)

        # ---- the cross-check against transformers ----
        hf = hf_model(c, state, int(inp["eos"]))
        res[f"hf_logits_{name}"] = np.float64(-1.0)
        if hf is not None:
            from transformers.modeling_outputs import BaseModelOutput
            worst = 0.0
            for b in range(3):
                xa = tt(inp["units"][b, : dnp.N_FRAMES[b]]).double()[None]
                tf = inp["tf_tokens"][b].copy()
                tf[dnp.TF_LEN[b]:] = 0
                lg = hf(encoder_outputs=BaseModelOutput(last_hidden_state=xa), decoder_input_ids=tt(tf)[None]).logits[0].numpy()
                worst = max(worst, float(np.abs(lg - l64[b]).max() / np.abs(l64[b]).max()))
                pl = len(inp["prompts"][b])
                n_new = len(gens[b][0]) - pl
                ids = hf.generate(encoder_outputs=BaseModelOutput(last_hidden_state=xa), decoder_input_ids=torch.tensor([inp["prompts"][b]]), max_new_tokens=n_new,
                                  do_sample=False, num_beams=1, suppress_tokens=list(inp["suppress"]), begin_suppress_tokens=list(inp["begin_suppress"]),
                                  eos_token_id=int(inp["eos"]), pad_token_id=int(inp["eos"]), return_timestamps=False)
                ids = np.asarray(ids[0] if not hasattr(ids, "sequences") else ids.sequences[0]).tolist()
                # (transformers' Whisper generate hands back the sequence without some or all of the prompt ids, depending on its version:
                #  the generated ids are what is compared, all of them)
                full = gens[b][0]
                assert n_new <= len(ids) <= len(full) and ids == full[len(full) - len(ids):], (name, b, ids, full)
            res[f"hf_logits_{name}"] = np.float64(worst)
            print(f"{name}: transformers agrees: logits within {worst:.2e} x absmax, greedy ids identical")
            assert worst < 1e-12

    np.savez_compressed(os.path.join(out, "whisper_decoder.npz"), **res)
    json.dump({"configs": dnp.CONFIGS, "shapes": manifest, "large_v3_dims": arch.WHISPER_LARGE_V3_DIMS},
              open(os.path.join(out, "manifest_whisper_decoder.json"), "w"), indent=0)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    if a.check:
        sys.exit(check())
    main(a.out)
