"""The Whisper text decoder at large-v3's dimensions, seeded weights, one process: B = 1 and B = 8 rows over 1500 encoder frames, 64 new
tokens from the 4-id prompt.  Per batch size: the `cross` call (every layer's cross keys and values), prefill + first step (a decode of one
token), microseconds per cached step ((64 tokens - 1 token) / 63), and each step's share of its traffic bound -- the bytes a step actually
reads (the blocks' weights once for all rows, the transposed embedding, the rows' cross and self caches) over the HBM bandwidth of the
MI355X (6.29 TB/s measured with a float4 copy, 8.0 TB/s by its data sheet).  With transformers present: WhisperForConditionalGeneration in
fp32 with the same weights on the same device in the same process, generate() with the same prompt and suppress list, alternating with
ours.  Warm-up, device events around whole calls, alternating rounds, minimum and spread; one JSON line, also written to --out.

    python tools/bench_whisper_decode.py [--layers 32] [--rounds 3] [--new-tokens 64] [--no-hf] [--out profiles/whisper_decode_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "latent-diffusion-speech_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lds import arch, init_weights, native  # noqa: E402

HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12
D = arch.WHISPER_LARGE_V3_DIMS
C, HEADS, V, CTX, T = D["n_text_state"], D["n_text_head"], D["n_vocab"], D["n_text_ctx"], D["n_audio_ctx"]


def step_bytes(layers, B, n_frames, self_keys):
    """what one cached step reads: per layer q|k|v 3 C^2, out C^2, cross query C^2, cross out C^2, the MLP 8 C^2 (the cross key / value
    weights are read by `cross` alone); the head's C x V; per row the cross keys and values of n_frames frames and the self caches"""
    w = layers * 14 * C * C * 4
    head = C * V * 4
    cross = B * layers * 2 * n_frames * C * 4
    own = B * layers * 2 * self_keys * C * 4
    return {"block_weights": w, "head": head, "cross_caches": cross, "self_caches": own, "total": w + head + cross + own}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def hf_model(state, layers, eos):
    try:
        from transformers import WhisperConfig, WhisperForConditionalGeneration
    except Exception as e:
        print("transformers is absent, the comparison is skipped:", e, file=sys.stderr)
        return None
    cfg = WhisperConfig(vocab_size=V, num_mel_bins=128, encoder_layers=1, encoder_attention_heads=HEADS, decoder_layers=layers, decoder_attention_heads=HEADS,
                        decoder_ffn_dim=4 * C, encoder_ffn_dim=4 * C, d_model=C, max_source_positions=T, max_target_positions=CTX, pad_token_id=eos,
                        bos_token_id=eos, eos_token_id=eos, decoder_start_token_id=0, suppress_tokens=None, begin_suppress_tokens=None,
                        activation_function="gelu", scale_embedding=False, dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, tie_word_embeddings=True)
    with torch.device("meta"):
        m = WhisperForConditionalGeneration(cfg)
    m = m.to_empty(device="cpu").float().eval()
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
            n = n.replace(".mlp.0.", ".fc1.").replace(".mlp.2.", ".fc2.").replace(".cross_attn.", ".encoder_attn.").replace(".attn.", ".self_attn.")
            n = n.replace(".query.", ".q_proj.").replace(".key.", ".k_proj.").replace(".value.", ".v_proj.").replace(".out.", ".out_proj.")
        sd["model.decoder." + n] = torch.from_numpy(v)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    for name, p in m.named_parameters():      # what the decoder's keys do not cover (the one-layer encoder, absent k_proj biases): zeros
        if name in missing:
            p.data.zero_()
    m.tie_weights()
    return m.cuda()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=D["n_text_layer"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--no-hf", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    t0 = time.time()
    state = arch.whisper_decoder_init_state(V, CTX, C, a.layers, 0)
    sp = arch.whisper_special_tokens(V)
    dec = native.WhisperDecoder(V, CTX, C, HEADS, a.layers, T, state)
    print(f"weights and handle: {time.time() - t0:.1f} s", file=sys.stderr)
    prompt1 = [sp["sot"], sp["languages"]["en"], sp["transcribe"], sp["notimestamps"]]
    units8 = torch.from_numpy(init_weights.uniform("bench.wdec.units", (8, T, C), 5, -1.7, 1.7)).cuda()
    eos = sp["eot"]
    ban = [eos]      # EOS suppressed: every row runs its 64 steps
    hf = None if a.no_hf else hf_model(state, a.layers, eos)
    del state
    out = {"layers": a.layers, "new_tokens": a.new_tokens, "n_frames": T, "hbm_measured_TBps": HBM_MEASURED / 1e12, "hbm_spec_TBps": HBM_SPEC / 1e12}
    for B in (1, 8):
        units = units8[:B].contiguous()
        ids = torch.tensor([prompt1] * B, dtype=torch.int64, device="cuda")
        plen = [4] * B
        legs = {
            "cross_ms": lambda: dec.cross(units, None, S=4 + a.new_tokens),
            "first_ms": lambda: dec.generate(ids, plen, 1, eos, eos, suppress=ban, cap=4 + a.new_tokens),
            "decode_ms": lambda: dec.generate(ids, plen, a.new_tokens, eos, eos, suppress=ban, cap=4 + a.new_tokens),
        }
        if hf is not None:
            from transformers.modeling_outputs import BaseModelOutput
            enc = BaseModelOutput(last_hidden_state=units)
            legs["hf_decode_ms"] = lambda: hf.generate(encoder_outputs=enc, decoder_input_ids=ids, max_new_tokens=a.new_tokens, do_sample=False, num_beams=1,
                                                       suppress_tokens=ban, begin_suppress_tokens=None, eos_token_id=eos, pad_token_id=eos, return_timestamps=False)
        for fn in legs.values():      # warm-up: every shape of the timed window
            fn()
        torch.cuda.synchronize()
        t = {k: [] for k in legs}
        for _ in range(a.rounds):     # alternating: every leg sees the same clocks and the same neighbours
            for k, fn in legs.items():
                t[k].append(timed(fn))
        r = {k: round(min(v), 3) for k, v in t.items()}
        r["spread_ms"] = {k: round(max(v) - min(v), 3) for k, v in t.items()}
        step_us = (min(t["decode_ms"]) - min(t["first_ms"])) / (a.new_tokens - 1) * 1e3
        by = step_bytes(a.layers, B, T, 4 + a.new_tokens // 2)
        r["step_us"] = round(step_us, 1)
        r["step_bytes"] = by
        r["bound_us_measured_bw"] = round(by["total"] / HBM_MEASURED * 1e6, 1)
        r["bound_us_spec_bw"] = round(by["total"] / HBM_SPEC * 1e6, 1)
        r["step_over_bound_measured_bw"] = round(step_us / (by["total"] / HBM_MEASURED * 1e6), 2)
        r["cross_cache_MB"] = round(2 * a.layers * B * T * C * 4 / 1e6, 1)
        if hf is not None:
            toks = dec.generate(ids, plen, a.new_tokens, eos, eos, suppress=ban, cap=4 + a.new_tokens)[0]
            theirs = legs["hf_decode_ms"]()
            theirs = theirs if torch.is_tensor(theirs) else theirs.sequences
            n = min(theirs.shape[1], a.new_tokens)
            r["hf_ids_equal"] = bool(torch.equal(theirs[:, -n:].cpu(), toks[:, -n:].cpu()))
            r["hf_over_native"] = round(r["hf_decode_ms"] / r["decode_ms"], 2)
        out[f"b{B}"] = r
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
