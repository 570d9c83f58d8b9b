"""The x-vector head's kernels (csrc/xvector.hip), one process, device events around whole calls after warm-up, alternating rounds, the
minimum of the rounds (and max - min as "spread"); one JSON line.

    python tools/bench_xvector.py [--rounds 5] [--iters 5] [--no-encode] [--layers 12]

  head     8 clips x 1499 frames, D = 768 and 1024: the whole native head (projector, five TDNN layers with the pooling in the last one's
           epilogue, join, two small linears) next to the same head restated in torch on the same device (linear, conv1d, relu, mean / std);
           "bar_met": native <= torch + the larger of the two spreads
  layers   every layer alone through the test entries, next to torch's linear / conv1d + relu of that layer (the last one with mean / std)
  encode   the head as a share of the 8 x 30 s WavLM encode it sits on (seeded weights, --layers deep), with and without the layer sum
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "latent-diffusion-speech_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from lds import native  # noqa: E402

B, T = 8, 1499


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def rounds(legs, n_rounds, iters):
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in legs}
    for _ in range(n_rounds):
        for k, fn in legs.items():
            t[k].append(timed(fn, iters))
    return {k: {"ms": round(min(v), 4), "spread_ms": round(max(v) - min(v), 4)} for k, v in t.items()}


def torch_layer(x, W, b, ks, dil, relu=True):
    """x [B, Cin, T] -> [B, Cout, T_out]: TDNNLayer.forward's conv1d of the viewed, transposed weight"""
    y = F.conv1d(x, W.view(W.shape[0], ks, -1).transpose(1, 2), b, dilation=dil)
    return F.relu(y) if relu else y


def torch_head(X, st, g):
    x = F.linear(X, st["projector.weight"], st["projector.bias"]).transpose(1, 2)
    for i, (ks, dil) in enumerate(zip(g["tdnn_kernel"], g["tdnn_dilation"])):
        x = torch_layer(x, st[f"tdnn.{i}.kernel.weight"], st[f"tdnn.{i}.kernel.bias"], ks, dil)
    stats = torch.cat([x.mean(dim=2), x.std(dim=2)], dim=1)
    emb = F.linear(stats, st["feature_extractor.weight"], st["feature_extractor.bias"])
    return emb, F.linear(emb, st["classifier.weight"], st["classifier.bias"])


def main():
    from encoder.xvector import XVectorHead
    from lds import arch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--no-encode", action="store_true")
    a = ap.parse_args()
    g = arch.XVECTOR_GEOMETRY
    res = {"B": B, "T": T}
    gen = torch.Generator(device="cuda").manual_seed(0)
    for D in (768, 1024):
        head = XVectorHead.synthetic(D, seed=0)
        h = head.native()
        st = {k: torch.from_numpy(v).cuda() for k, v in head._state.items()}
        X = torch.randn(B, T, D, device="cuda", generator=gen)
        nf = [T] * B
        # (the nominal count: every layer at T frames, ignoring the 14 that the valid convolutions lose)
        flops = 2.0 * B * T * (D * 512 + sum(c * k * ci for c, k, ci in zip(g["tdnn_dim"], g["tdnn_kernel"], (512,) + g["tdnn_dim"][:-1])))
        r = rounds({"native": lambda: h.embed(X, nf), "torch": lambda: torch_head(X, st, g)}, a.rounds, a.iters)
        r["native_tflops"] = round(flops / r["native"]["ms"] / 1e9, 2)
        r["bar_met"] = bool(r["native"]["ms"] <= r["torch"]["ms"] + max(r["native"]["spread_ms"], r["torch"]["spread_ms"]))
        e_n, e_t = h.embed(X, nf)[0], torch_head(X, st, g)[0]
        r["native_vs_torch_relmax"] = float((e_n - e_t).abs().max() / e_t.abs().max())
        res[f"head_D{D}"] = r
        # per layer
        per = {}
        x = X
        specs = [("projector", "projector", 1, 1, False)] + [(f"tdnn{i}", f"tdnn.{i}.kernel", k, d, True) for i, (k, d) in enumerate(zip(g["tdnn_kernel"], g["tdnn_dilation"]))]
        n_in = T
        for name, key, ks, dil, relu in specs:
            W, b = st[key + ".weight"], st[key + ".bias"]
            last = name == f"tdnn{len(g['tdnn_dim']) - 1}"
            xin, xt, lens = x, x[:, :n_in].transpose(1, 2).contiguous(), [n_in] * B
            if last:
                def tl(xt=xt, W=W, b=b, ks=ks, dil=dil):
                    y = torch_layer(xt, W, b, ks, dil)
                    return y.mean(dim=2), y.std(dim=2)
                legs = {"native": lambda xin=xin, lens=lens, W=W, b=b, ks=ks, dil=dil: native.xvector_test_pool(xin, lens, W, b, ks, dil), "torch": tl}
            else:
                legs = {"native": lambda xin=xin, lens=lens, W=W, b=b, ks=ks, dil=dil, relu=relu: native.xvector_test_tdnn(xin, lens, W, b, ks, dil, relu=relu),
                        "torch": lambda xt=xt, W=W, b=b, ks=ks, dil=dil, relu=relu: torch_layer(xt, W, b, ks, dil, relu)}
            q = rounds(legs, a.rounds, a.iters)
            q["native_tflops"] = round(2.0 * B * (n_in - (ks - 1) * dil) * W.numel() / q["native"]["ms"] / 1e9, 2)
            per[name] = q
            if not last:
                x = native.xvector_test_tdnn(xin, lens, W, b, ks, dil, relu=relu)
                n_in -= (ks - 1) * dil
        res[f"layers_D{D}"] = per
    if not a.no_encode:
        from encoder.xvector import SpeakerEncoder
        from lds import init_weights
        from tools.tools import WavLMUnits
        dims = dict(arch.wavlm_dims("base+"), n_layer=a.layers)
        units = WavLMUnits.synthetic("wavlmbase+", dims, seed=0, device="cuda")
        audio = torch.from_numpy(init_weights.uniform("bench.xvector.audio", (B, 480000), 5, -0.5, 0.5)).cuda()
        lens = [480000] * B
        spk_sum = SpeakerEncoder(units, XVectorHead.synthetic(768, seed=0, n_layer=a.layers))
        spk_last = SpeakerEncoder(units, XVectorHead.synthetic(768, seed=0))
        lw = spk_sum.head.layer_weights
        r = rounds({"encode": lambda: units.model.encode(audio, lens), "encode_layersum": lambda: units.model.encode(audio, lens, layer_weights=lw),
                    "embed_last": lambda: spk_last.embed_audio(audio, lens), "embed_layersum": lambda: spk_sum.embed_audio(audio, lens)}, max(2, a.rounds // 2), 1)
        r["head_share_last"] = round(r["embed_last"]["ms"] / r["encode"]["ms"] - 1, 4)
        r["head_share_layersum"] = round(r["embed_layersum"]["ms"] / r["encode_layersum"]["ms"] - 1, 4)
        r["layersum_over_encode"] = round(r["encode_layersum"]["ms"] / r["encode"]["ms"] - 1, 4)
        r["layers"] = a.layers
        res["encode_8x30s_wavlm_base"] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
