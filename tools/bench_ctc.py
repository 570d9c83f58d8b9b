"""The CTC head's kernels (csrc/ctc.hip), one process, device events around whole calls after warm-up, alternating rounds, the minimum of the
rounds (and max - min as "spread"); one JSON line.

    python tools/bench_ctc.py [--rounds 5] [--iters 5] [--no-transcribe] [--layers 24]

  head       statistics at N = 12,000 (8 x 1500), D = 1024, V = 32 and 4096, next to lds_kmeans_assign at K = V (the kernel of the same tiling:
             the head's extra work is the exp / log epilogue and the fixed 4-block column splits) and next to torch's F.linear + log_softmax
             + argmax on the same device; also the head with log-probs stored
  recursion  score and align for 8 clips of 1499 frames with L = 100 and 500 (head + gathered emissions + recursion), the recursion alone
             through the test entries on ready emissions (us per frame), next to torch.nn.functional.ctc_loss on the device given ready
             log-probs
  transcribe head + collapse on top of an 8 x 30 s XLSR encode (seeded weights, --layers deep), as a share of the encode
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "latent-diffusion-speech_amd"))
import torch  # noqa: E402

from lds import native  # noqa: E402

D = 1024


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--no-transcribe", action="store_true")
    a = ap.parse_args()
    res = {"D": D}
    g = torch.Generator(device="cuda").manual_seed(0)
    B, T = 8, 1500
    X = torch.randn(B, T, D, device="cuda", generator=g)
    nf = [T] * B
    for V in (32, 4096):
        W = torch.randn(V, D, device="cuda", generator=g) / D ** 0.5
        b = torch.randn(V, device="cuda", generator=g)
        h = native.kmeans_prepare(W)
        X2 = X.reshape(-1, D)

        def torch_ref():
            lp = torch.nn.functional.linear(X2, W, b).log_softmax(-1)
            return lp, lp.argmax(-1)

        legs = {"head": lambda: native.ctc_head(X, nf, W, b), "kmeans_assign": lambda: native.kmeans_assign(X2, W, h, return_best=True),
                "head_logprobs": lambda: native.ctc_head(X, nf, W, b, return_logprobs=True), "torch_linear_log_softmax_argmax": torch_ref}
        r = rounds(legs, a.rounds, a.iters)
        r["head_over_assign"] = round(r["head"]["ms"] / r["kmeans_assign"]["ms"], 3)
        r["head_tflops"] = round(2.0 * B * T * V * D / r["head"]["ms"] / 1e9, 2)
        res[f"head_N{B * T}_V{V}"] = r
    # the recursions
    T, V = 1499, 32
    X = torch.randn(B, T, D, device="cuda", generator=g)
    W = torch.randn(V, D, device="cuda", generator=g) / D ** 0.5
    b = torch.randn(V, device="cuda", generator=g)
    nf = [T] * B
    lp = native.ctc_head(X, nf, W, b, return_logprobs=True)[3]
    lp_t = lp.transpose(0, 1).contiguous()
    for L in (100, 500):
        labels = torch.randint(1, V, (B, L), device="cuda", generator=g)
        ll = [L] * B
        E = torch.cat([lp[:, :, :1], torch.gather(lp, 2, labels[:, None, :].expand(B, T, L))], dim=2).contiguous()
        tl, il = torch.tensor(ll), torch.tensor(nf)
        legs = {"score": lambda: native.ctc_score(X, nf, W, b, 0, labels, ll), "align": lambda: native.ctc_align(X, nf, W, b, 0, labels, ll),
                "forward_alone": lambda: native.ctc_test_forward(E, nf, labels, ll), "viterbi_alone": lambda: native.ctc_test_viterbi(E, nf, labels, ll),
                "torch_ctc_loss": lambda: torch.nn.functional.ctc_loss(lp_t, labels, il, tl, blank=0, reduction="none")}
        r = rounds(legs, a.rounds, a.iters)
        r["forward_us_per_frame"] = round(r["forward_alone"]["ms"] * 1e3 / T, 4)
        r["viterbi_us_per_frame"] = round(r["viterbi_alone"]["ms"] * 1e3 / T, 4)
        res[f"recursion_B{B}_T{T}_L{L}"] = r
    if not a.no_transcribe:
        from encoder.ctc import CTCHead
        from lds import arch, init_weights
        from tools.tools import Audio2xlsr_53_56k
        enc = Audio2xlsr_53_56k.synthetic(dict(arch.XLSR_53_DIMS, n_layer=a.layers), seed=0, device="cuda")
        head = CTCHead.synthetic(enc.hidden_dim, 32, seed=0)
        audio = torch.from_numpy(init_weights.uniform("bench.ctc.audio", (8, 480000), 5, -0.5, 0.5)).cuda()
        lens = [480000] * 8
        nfr = [enc.frames_of(480000)] * 8
        w, bb = head._w.cuda(), head._b.cuda()

        def transcribe():
            units, _ = enc.encode_ragged(audio, lens)
            return native.ctc_greedy(*native.ctc_head(units, nfr, w, bb), nfr, 0)

        r = rounds({"encode": lambda: enc.encode_ragged(audio, lens), "encode_transcribe": transcribe}, max(2, a.rounds // 2), 1)
        r["share_on_top"] = round(r["encode_transcribe"]["ms"] / r["encode"]["ms"] - 1, 4)
        r["layers"] = a.layers
        res["transcribe_8x30s_xlsr"] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
