"""The k-means tokenizer's kernels at the reference's configuration (K 4096 centres of 1280 floats), one process, device events around whole
calls after warm-up, alternating rounds, the minimum of the rounds; one JSON line.

    python tools/bench_kmeans.py [--rounds 3] [--iters 3] [--big 1000000] [--no-tokens] [--no-fit] [--metric cosine]

  assign    N = 1500, 12,000 and --big rows: time and 2 N K D / time (a kernel figure), next to the same product (M 4096, K 1280, N columns) as a
            plain conv_dma 1x1 launch that STORES the N x K result (include/lds_test.h lds_bench_dconv, the mechanism of tools/bench_dconv.py)
            and, for information, torch's 2 a @ b.T - ... + max (the reference's formula) on the same device
  update    one Lloyd step at --big rows against N D 4 bytes / time
  fit       one iteration (assign + update) at --big rows; KMeansGPU.fit_predict on a seeded blob corpus of that size (max_iter 5), the
            seeding timed separately
  tokens    assign of 8 x 1500 frames on top of an 8-clip, 30 s Whisper encode (large-v3 dims, seeded weights)
  --metric cosine   the cosine assign (with its similarities) and the cosine Lloyd step join the same alternating rounds as legs of their
            own: "cosine_ms" beside "ms", with the (max - min) of both legs' rounds; the fit then runs KMeansCosineGPU
"""
import argparse
import ctypes as ct
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "latent-diffusion-speech_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lds import native  # noqa: E402

PEAK_TFLOPS = 157.3
K, D = 4096, 1280


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
    rounds.spread = {k: max(v) - min(v) for k, v in t.items()}
    return {k: min(v) for k, v in t.items()}


def dconv_ms(B, T, w, iters):
    """the plain conv_dma 1x1 launch of the same product, result stored: ms per launch"""
    x = torch.randn(B, D, T, device="cuda")
    out = torch.empty(B, K, T, device="cuda")
    a = native.DConvTest()
    a.x1, a.x2, a.C1, a.C2, a.T = x.data_ptr(), None, D, 0, T
    a.w, a.bias, a.Co, a.K, a.stride, a.pad, a.ups = w.ctypes.data, None, K, 1, 1, 0, 0
    a.res, a.epilogue, a.plain_out, a.v_split, a.cfg = None, 0, 0, 0, 0
    ms, cs = ct.c_float(), ct.create_string_buffer(128)
    native.check(native.lib().lds_bench_dconv(ct.byref(a), ct.c_void_p(out.data_ptr()), B, iters, ct.byref(ms), cs, 128,
                                              ct.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return ms.value, cs.value.decode()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--big", type=int, default=1000000)
    ap.add_argument("--no-tokens", action="store_true")
    ap.add_argument("--no-fit", action="store_true")
    ap.add_argument("--metric", default="l2", choices=("l2", "cosine"))
    a = ap.parse_args()
    cos = a.metric == "cosine"
    res = {"K": K, "D": D, "peak_tflops": PEAK_TFLOPS}
    g = torch.Generator(device="cuda").manual_seed(0)
    C = torch.randn(K, D, device="cuda", generator=g)
    h = native.kmeans_prepare(C)
    hr = native.kmeans_prepare(C, "cosine") if cos else None
    lab_true = torch.randint(0, K, (a.big,), device="cuda", generator=g)
    Xbig = C[lab_true] + 0.5 * torch.randn(a.big, D, device="cuda", generator=g)
    w = np.ascontiguousarray(C.cpu().numpy().reshape(K, D, 1))
    shapes = {1500: (1, 1500), 12000: (8, 1500), a.big: (64, a.big // 64)}
    for N in (1500, 12000, a.big):
        X = Xbig[:N].contiguous()

        def torch_ref():
            for r0 in range(0, N, 65536):      # (chunked: the N x K matrix of a million rows is 16 GB)
                x = X[r0:r0 + 65536]
                (2 * x @ C.T - (x ** 2).sum(1)[:, None] - (C ** 2).sum(1)[None, :]).max(-1)

        legs = {"assign": lambda: native.kmeans_assign(X, C, h), "torch": torch_ref}
        if cos:
            legs["assign_cosine"] = lambda: native.kmeans_assign(X, C, hr, return_best=True, metric="cosine")
        ms = rounds(legs, a.rounds, a.iters)
        B, T = shapes[N]
        try:
            dms = [dconv_ms(B, T, w, a.iters) for _ in range(a.rounds)]
        except RuntimeError as e:      # (a shape the single-op entry refuses: reported, the other legs still count)
            res[f"assign_{N}_conv_dma_error"] = str(e)[:200]
            dms = [(float("nan"), "")]
        fl = 2.0 * N * K * D
        dfl = 2.0 * B * T * K * D
        res[f"assign_{N}"] = {"ms": round(ms["assign"], 4), "tflops": round(fl / ms["assign"] / 1e9, 1), "frac_peak": round(fl / ms["assign"] / 1e9 / PEAK_TFLOPS, 3),
                              "conv_dma_ms": round(min(m for m, _ in dms), 4), "conv_dma_tflops": round(dfl / min(m for m, _ in dms) / 1e9, 1),
                              "conv_dma_cfg": dms[0][1], "conv_dma_columns": B * T,
                              "assign_over_conv_dma_per_flop": round((ms["assign"] / fl) / (min(m for m, _ in dms) / dfl), 3),
                              "torch_ms": round(ms["torch"], 4)}
        if cos:
            res[f"assign_{N}"].update({"cosine_ms": round(ms["assign_cosine"], 4), "spread_ms": round(rounds.spread["assign"], 4),
                                       "cosine_spread_ms": round(rounds.spread["assign_cosine"], 4)})
    # the Lloyd step and one fit iteration at --big rows
    N = a.big
    labels = native.kmeans_assign(Xbig, C, h)
    npnt = torch.ones(K, device="cuda")
    C2, h2 = C.clone(), h.clone()
    step = lambda: native.kmeans_update(Xbig, labels, C2, h2, npnt)      # noqa: E731
    it = lambda: native.kmeans_update(Xbig, native.kmeans_assign(Xbig, C2, h2), C2, h2, npnt)      # noqa: E731
    legs = {"update": step, "iteration": it}
    if cos:
        C3, h3 = C.clone(), hr.clone()
        legs["iteration_cosine"] = lambda: native.kmeans_update(Xbig, native.kmeans_assign(Xbig, C3, h3, metric="cosine"), C3, h3, npnt, metric="cosine")
    ms = rounds(legs, a.rounds, a.iters)
    res[f"update_{N}"] = {"ms": round(ms["update"], 4), "x_bytes_per_s_TB": round(N * D * 4 / ms["update"] / 1e9, 3)}
    res[f"iteration_{N}"] = {"ms": round(ms["iteration"], 4)}
    if cos:
        res[f"iteration_{N}"].update({"cosine_ms": round(ms["iteration_cosine"], 4), "spread_ms": round(rounds.spread["iteration"], 4),
                                      "cosine_spread_ms": round(rounds.spread["iteration_cosine"], 4)})
    if not a.no_fit:
        from cluster.kmeans import KMeansCosineGPU, KMeansGPU, _kpp
        torch.manual_seed(0)
        km = (KMeansCosineGPU if cos else KMeansGPU)(K, max_iter=5, tol=0.0)
        t0 = time.perf_counter()
        km.fit_predict(Xbig)
        torch.cuda.synchronize()
        t_fit = time.perf_counter() - t0
        offset = np.power(1.5, np.log(K / 1000)) / np.log(2)
        n_seed = min(int(km.minibatch / 12 / offset), N)
        torch.manual_seed(0)
        t0 = time.perf_counter()
        _kpp(Xbig, K, n_seed)
        torch.cuda.synchronize()
        t_seed = time.perf_counter() - t0
        res[f"fit_predict_{N}"] = {"wall_s_5_iterations_with_seeding": round(t_fit, 3), "seeding_wall_s": round(t_seed, 3), "seeding_rows": n_seed,
                                   "minibatch": km.minibatch}
    if not a.no_tokens:
        from lds import arch, init_weights
        hw = native.Whisper(128, 1280, 20, 32, 1500, arch.whisper_init_state(128, 1280, 32, 0), arch.whisper_mel_filters(128))
        audio = torch.from_numpy(init_weights.uniform("bench.units.audio", (8, 480000), 5, -0.5, 0.5)).cuda()
        enc = lambda: hw.encode(audio)      # noqa: E731
        tok = lambda: native.kmeans_assign(hw.encode(audio).reshape(-1, D), C, h)      # noqa: E731
        ms = rounds({"encode": enc, "encode_tokens": tok}, a.rounds, 1)
        res["tokens_8x30s"] = {"encode_ms": round(ms["encode"], 3), "encode_tokens_ms": round(ms["encode_tokens"], 3),
                               "share_on_top": round(ms["encode_tokens"] / ms["encode"] - 1, 4)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
