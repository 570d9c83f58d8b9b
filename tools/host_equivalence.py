"""What the library's host side answers, as one JSON document, so that two builds can be compared field by field:

    python tools/host_equivalence.py PATH/TO/liblds.so > doc.json      # one fresh process per library

  workspace_bytes  every *_workspace_bytes entry at a small and a large argument set, and lds_debug_unet_plan's text
  outputs          SHA-256 of the outputs of one small call per component whose create or plan is written on csrc/host.h
  refusals         (rc, message) of refused calls: the argument checks that live in host.h and a missing / wrong-size tensor per create

The handle-free part needs no GPU; everything behind a create does ("gpu": false leaves it out).  Weights are the seeded init states
of lds/arch.py, inputs are seeded too, so two documents of one build are equal."""
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "latent-diffusion-speech_amd"))
from lds import arch, init_weights, native  # noqa: E402

DOC = {"workspace_bytes": {}, "outputs": {}, "refusals": {}}
L = None


def size(entry, *args):
    nb = C.c_size_t()
    rc = getattr(L, entry)(*args, C.byref(nb))
    DOC["workspace_bytes"][f"{entry}{[a for a in args if isinstance(a, int)]}"] = nb.value if rc == 0 else [rc, L.lds_last_error().decode()]


def refusal(tag, fn):
    """fn: a call that must be refused, through the ctypes entry (returns rc) or through a native wrapper (raises RuntimeError)"""
    try:
        rc = fn()
        DOC["refusals"][tag] = [rc, L.lds_last_error().decode()] if isinstance(rc, int) and rc else "accepted"
    except RuntimeError as e:
        DOC["refusals"][tag] = str(e)


def out(tag, *tensors):
    import torch
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        if t is not None:
            h.update(t.detach().cpu().contiguous().numpy().tobytes())
    DOC["outputs"][tag] = h.hexdigest()


def U(tag, shape, lo=-1.0, hi=1.0):
    return init_weights.uniform("equiv." + tag, shape, 7, lo, hi)


def handle_free():
    for N, K, D in ((1000, 100, 64), (200000, 4096, 768)):
        size("lds_kmeans_workspace_bytes", N, K, D)
    for N, M, D, k in ((77, 1000, 64, 4), (16384, 500000, 768, 8)):
        size("lds_knn_workspace_bytes", N, M, D, k)
        size("lds_ivf_workspace_bytes", N, M, D, k, 32 if M == 1000 else 1024, 4 if M == 1000 else 8)
    for B, T, V, D, Lm in ((3, 50, 40, 64, 12), (16, 1500, 32000, 1024, 200)):
        size("lds_ctc_head_workspace_bytes", B, T, V, D)
        size("lds_ctc_score_workspace_bytes", B, T, V, D, Lm)
        size("lds_ctc_align_workspace_bytes", B, T, V, D, Lm)
        size("lds_test_xvector_pool_workspace_bytes", B, T, 1500 if D > 64 else 64)
    size("lds_stft_mel_workspace_bytes", 2048, 512, 128, 2, 44100)
    size("lds_stft_mel_workspace_bytes", 2048, 512, 128, 16, 441000)
    size("lds_loss_reduce_workspace_bytes", 1000)
    size("lds_loss_reduce_workspace_bytes", 16 * 80 * 512)
    nb = C.c_size_t()
    i3, bad = (C.c_int32 * 3)(5, 0, 9), (C.c_int32 * 3)(5, 10, 9)
    refusal("ctc_head_ws B=65", lambda: L.lds_ctc_head_workspace_bytes(65, 50, 40, 64, C.byref(nb)))
    refusal("ctc_head_ws V=1", lambda: L.lds_ctc_head_workspace_bytes(3, 50, 1, 64, C.byref(nb)))
    refusal("ctc_head_ws T=0", lambda: L.lds_ctc_head_workspace_bytes(3, 0, 40, 64, C.byref(nb)))
    refusal("ctc_score_ws Lmax=0", lambda: L.lds_ctc_score_workspace_bytes(3, 50, 40, 64, 0, C.byref(nb)))
    refusal("ctc_greedy B=0", lambda: L.lds_ctc_greedy(None, None, None, 0, 9, i3, 0, -1, None, None, None, None, None, None))
    refusal("ctc_greedy null n_frames", lambda: L.lds_ctc_greedy(None, None, None, 3, 9, None, 0, -1, None, None, None, None, None, None))
    refusal("ctc_greedy n_frames[1]=10", lambda: L.lds_ctc_greedy(None, None, None, 3, 9, bad, 0, -1, None, None, None, None, None, None))
    refusal("ctc_score label_len[1]=10", lambda: L.lds_ctc_score(None, 3, 9, i3, None, None, 40, 64, 0, None, bad, 9, None, None, 0, None))
    refusal("ctc_score null label_len", lambda: L.lds_ctc_score(None, 3, 9, i3, None, None, 40, 64, 0, None, None, 9, None, None, 0, None))
    refusal("xvector_pool_ws B=65", lambda: L.lds_test_xvector_pool_workspace_bytes(65, 50, 64, C.byref(nb)))
    refusal("xvector_pool_ws T=0", lambda: L.lds_test_xvector_pool_workspace_bytes(3, 0, 64, C.byref(nb)))
    refusal("xvector_pool_ws T=32769", lambda: L.lds_test_xvector_pool_workspace_bytes(3, 32769, 64, C.byref(nb)))
    refusal("xvector_tdnn n_frames[1]=10", lambda: L.lds_test_xvector_tdnn(None, 3, 9, bad, None, None, 64, 64, 3, 1, 1, None, None))
    refusal("xvector_tdnn null n_frames", lambda: L.lds_test_xvector_tdnn(None, 3, 9, None, None, None, 64, 64, 3, 1, 1, None, None))
    knn = (None, None, 1000, 64, 4, 0.5, None, None, None, None, 0, None)
    refusal("knn_retrieve_ragged B=65", lambda: L.lds_knn_retrieve_ragged(None, 65, 9, i3, *knn))
    refusal("knn_retrieve_ragged null lengths", lambda: L.lds_knn_retrieve_ragged(None, 3, 9, None, *knn))
    refusal("knn_retrieve_ragged lengths[1]=10", lambda: L.lds_knn_retrieve_ragged(None, 3, 9, bad, *knn))
    # the encoders' dimension rules refuse a create before it touches a device; plan_bytes and clip_lens_check refuse before they need a handle
    hub = dict(arch.HUBERT_BASE_DIMS)
    for tag, d in (("width_check capped conv_dim=100", dict(hub, conv_dim=100)), ("width_check n_ffn=100", dict(hub, n_ffn=100)),
                   ("heads_check n_head=5", dict(hub, n_head=5)), ("range_check n_layer=0", dict(hub, n_layer=0)),
                   ("range_check n_ctx=1501", dict(hub, n_ctx=1501))):
        cfg, h = native.HubertCfg(*(d[k] for k in native.Hubert.FIELDS)), C.c_void_p()
        refusal("hubert_create " + tag, lambda: L.lds_hubert_create(C.byref(cfg), 0, (C.c_char_p * 1)(), (C.c_void_p * 1)(), (C.c_int64 * 1)(), C.byref(h)))
    refusal("plan_bytes null out", lambda: L.lds_hubert_workspace_bytes(None, 3, 16000, 40, None))
    l65 = (C.c_int32 * 65)(*([512] * 65))
    refusal("clip_lens_check B=65", lambda: L.lds_vae_encoder_forward_ragged(None, None, l65, None, None, None, 0, None, 0, 65, 512, None))


def last_1d(state):
    """a one-dimensional tensor every create reads: the last one of the second layer"""
    return [k for k, v in state.items() if v.ndim == 1 and ".1." in k][-1]


def creates(name, make, state, key_1d):
    """a missing and a wrong-size tensor of one create; key_1d names a one-dimensional tensor of `state`"""
    refusal(f"{name}_create missing", lambda: make({k: v for k, v in state.items() if k != key_1d}))
    refusal(f"{name}_create wrong size", lambda: make(dict(state, **{key_1d: state[key_1d][:-1]})))


def with_gpu():
    import numpy as np
    import torch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    ints = lambda tag, shape, hi: dev((U(tag, shape, 0, 1) * hi).astype(np.int64))      # noqa: E731

    # RoFormer LM
    def lm():
        c = arch.roformer_config()
        st = arch.roformer_init_state(c, 0)
        lm = native.LM(c, st)
        for a in ((2, 9, 24), (8, 64, 513)):
            size("lds_lm_workspace_bytes", lm.h, *a)
            size("lds_lm_workspace_bytes_opts", lm.h, *a, 4)
            size("lds_lm_workspace_bytes_prompt", lm.h, *a, 5)
            size("lds_lm_score_workspace_bytes", lm.h, a[0], a[1], a[2] - 1)
        creates("lm", lambda s: native.LM(c, s), st, "semantic_decoder.cls.predictions.transform.LayerNorm.bias")
        enc = lm.encode(ints("lm.phone", (2, 9), 100), ints("lm.tone", (2, 9), 10), ints("lm.spk", (2, 1), 300))
        out("lm.generate greedy", *lm.generate(enc, 24, False, 0, 1.0, 1.0, 1.2, return_logits=True))
        out("lm.generate beam", *lm.generate(enc, 24, False, 0, 1.0, 1.0, 1.2, num_beams=4, no_repeat_ngram_size=3))
        prompt = torch.cat([torch.full((2, 1), c["sem_bos"], dtype=torch.int64, device="cuda"), ints("lm.prompt", (2, 4), 4000)], 1)
        out("lm.generate_prompt", *lm.generate_prompt(enc, prompt, [5, 3], 24, False, 0, 1.0, 1.0, 1.2, return_logits=True))
        out("lm.score", *lm.score(enc, ints("lm.sem", (2, 17), 4000), return_logits=True))
        del lm

    # Llama LM
    def llama():
        c = arch.llama_config(semantic_kmeans_num=512, hidden_size=256, num_attention_heads=4, num_key_value_heads=2, intermediate_size=512,
                              num_hidden_layers=2, max_position_embeddings=256)
        st = arch.llama_init_state(c, 0)
        ll = native.Llama(c, st)
        for a in ((2, 7, 24), (8, 64, 200)):
            size("lds_llama_workspace_bytes", ll.h, *a)
            size("lds_llama_beam_workspace_bytes", ll.h, *a, 4)
            size("lds_llama_score_workspace_bytes", ll.h, a[0], a[2])
        creates("llama", lambda s: native.Llama(c, s), st, "llama.model.norm.weight")
        ids = ints("ll.ids", (2, 7), 100) + 3
        out("llama.generate", *ll.generate(ids, [7, 5], 24, False, 0, 1.0, 1.0, 1.2, return_logits=True))
        out("llama.generate_beam", ll.generate_beam(ids, [7, 5], 24, 3))
        out("llama.score", *ll.score(ints("ll.score", (2, 19), c["vocab"] - 1), return_logits=True))
        refusal("llama.generate in_len[1]=9", lambda: ll.generate(ids, [7, 9], 24, False, 0, 1.0, 1.0, 1.0))
        del ll

    # x-vector head
    def xvector():
        g = dict(tdnn_dim=(64, 64), tdnn_kernel=(3, 1), tdnn_dilation=(2, 1), xvector_output_dim=32)
        st = arch.xvector_init_state(64, 0, None, 8, g)
        mk = lambda s, d_in=64: native.XVector(d_in, g["tdnn_dim"], g["tdnn_kernel"], g["tdnn_dilation"], 32, s)      # noqa: E731
        xv = mk(st)
        size("lds_xvector_workspace_bytes", xv.h, 3, 150)
        size("lds_xvector_workspace_bytes", xv.h, 16, 1500)
        creates("xvector", mk, st, "tdnn.1.kernel.bias")
        refusal("xvector_create no classifier.bias", lambda: mk({k: v for k, v in st.items() if k != "classifier.bias"}))
        refusal("xvector_create wrong d_in", lambda: mk(st, 96))
        DOC["outputs"]["xvector.n_labels"] = xv.n_labels
        out("xvector.embed", *xv.embed(dev(U("xv.x", (3, 150, 64))), [150, 6, 77]))
        nb, n3 = C.c_size_t(), (C.c_int32 * 3)(150, 6, 151)
        refusal("xvector_embed B=65", lambda: L.lds_xvector_embed(xv.h, None, n3, None, None, None, 0, 65, 150, None))
        refusal("xvector_embed T=0", lambda: L.lds_xvector_embed(xv.h, None, n3, None, None, None, 0, 3, 0, None))
        refusal("xvector_embed n_frames[2]=151", lambda: L.lds_xvector_embed(xv.h, None, n3, None, None, None, 0, 3, 150, None))
        refusal("xvector_embed null n_frames", lambda: L.lds_xvector_embed(xv.h, None, None, None, None, None, 0, 3, 150, None))
        del xv

    # CTC, k-NN, IVF, k-means: the plans written on Slots
    def plans():
        units, W, b = dev(U("ctc.x", (3, 50, 64))), dev(U("ctc.w", (40, 64))), dev(U("ctc.b", (40,)))
        nf, labels, ll_ = [50, 0, 33], ints("ctc.lab", (3, 12), 39) + 1, [12, 0, 5]
        arg, m, lse = native.ctc_head(units, nf, W, b)
        out("ctc.head", arg, m, lse)
        out("ctc.greedy", *native.ctc_greedy(arg, m, lse, nf, 0))
        out("ctc.score", native.ctc_score(units, nf, W, b, 0, labels, ll_))
        out("ctc.align", *native.ctc_align(units, nf, W, b, 0, labels, ll_))
        x, pool = dev(U("knn.x", (3, 26, 64))), dev(U("knn.pool", (1000, 64)))
        h = native.knn_prepare(pool)
        out("knn.search", *native.knn_search(x.reshape(-1, 64), pool, h, 4))
        out("knn.retrieve", *native.knn_retrieve(x.reshape(-1, 64), pool, h, 4, 0.5))
        out("knn.retrieve ragged", *native.knn_retrieve(x, pool, h, 4, 0.5, lengths=[26, 0, 7]))
        from cluster.index import UnitsIndex
        ix = UnitsIndex(pool).build_ivf(16, seed=0)
        out("ivf.search", *ix.search(x.reshape(-1, 64), k=4, nprobe=4))
        out("ivf.retrieve ragged", *ix.retrieve(x, k=4, ratio=0.5, lengths=[26, 0, 7], return_neighbours=True, nprobe=4))
        cent = dev(U("km.c", (100, 64)))
        hk = native.kmeans_prepare(cent)
        xs = dev(U("km.x", (1000, 64)))
        lab = native.kmeans_assign(xs, cent, hk)
        out("kmeans.assign", lab)
        npts = torch.zeros(100, device="cuda")
        out("kmeans.update", native.kmeans_update(xs, lab, cent, hk, npts), cent, hk, npts)
        out("kmeans.seed", *native.kmeans_seed(xs, 16, 3, dev(U("km.u", (15,), 0, 1))))

    # UNet: the arena with its slot log
    def unet():
        cfg = arch.unet_config()
        ust = init_weights.init_state(arch.unet_param_shapes(cfg), 0)
        u = native.UNet(cfg, ust)
        for B, T in ((2, 77), (16, 512)):
            size("lds_unet_workspace_bytes", u.h, B, T)
            size("lds_sampler_workspace_bytes", u.h, B, T)
            DOC["workspace_bytes"][f"lds_debug_unet_plan[{B}, {T}]"] = hashlib.sha256(repr(u.plan(B, T)).encode()).hexdigest()
        creates("unet", lambda s: native.UNet(cfg, s), ust, "conv_in.bias")
        out("unet.forward", u.forward(dev(U("unet.x", (2, u.M, 77), -2, 2)), dev(U("unet.c", (2, u.H, 77))), dev(np.array([321.25, 17.0], dtype=np.float32))))
        del u
        hv = arch.SYNTHETIC_VOCODER_H
        gst = init_weights.init_state(arch.generator_param_shapes(hv), 0)
        gen = native.Generator(hv, gst)
        size("lds_vocoder_workspace_bytes", gen.h, 2, 77)
        size("lds_vocoder_workspace_bytes", gen.h, 16, 512)
        creates("vocoder", lambda s: native.Generator(hv, s), gst, "conv_pre.weight_g")      # (its biases are optional)
        est = init_weights.init_state(arch.encoder_param_shapes(hv), 0)
        vae = native.VaeEncoder(hv, est)
        size("lds_vae_encoder_workspace_bytes", vae.h, 2, 77 * vae.hop)
        size("lds_vae_encoder_workspace_bytes", vae.h, 16, 512 * vae.hop)
        creates("vae_encoder", lambda s: native.VaeEncoder(hv, s), est, [k for k in est if k.endswith(".bias")][-1])
        emb = native.Embed(U("embed.w", (256, 1280)), U("embed.b", (256,)), U("embed.spk", (324, 256)))
        size("lds_embed_workspace_bytes", emb.h, 2, 77)
        size("lds_embed_workspace_bytes", emb.h, 16, 512)
        del gen, vae, emb

    # the units encoders (WeightLoader / plan_bytes / clip_lens_check since the earlier toolkit change): HuBERT ragged, the others' sizes
    def encoders():
        d = dict(arch.HUBERT_BASE_DIMS, n_layer=2)
        st = arch.hubert_init_state(d, 0)
        hb = native.Hubert(d, st)
        size("lds_hubert_workspace_bytes", hb.h, 3, 16000, 40)
        size("lds_hubert_workspace_bytes", hb.h, 16, 480000, 40)
        creates("hubert", lambda s: native.Hubert(d, s), st, last_1d(st))
        audio = dev(U("hubert.audio", (3, 16000)))
        out("hubert.encode ragged", hb.encode(audio, lengths=[16000, 400, 9999]))
        short, a = (C.c_int32 * 3)(16000, 319, 9999), C.c_void_p(audio.data_ptr())      # refused before anything is read or launched
        refusal("clip_lens_check length[1]=319", lambda: L.lds_hubert_encode(hb.h, a, short, a, 2, 0, a, 0, 3, 16000, 40, None))
        refusal("range_check B=0", lambda: L.lds_hubert_workspace_bytes(hb.h, 0, 16000, 40, C.byref(C.c_size_t())))
        del hb
        for name, cls, d, init in (("w2v", native.Wav2Vec2, dict(arch.XLSR_53_DIMS, n_layer=2), arch.w2v_init_state),
                                   ("wavlm", native.WavLM, dict(arch.wavlm_dims("base+"), n_layer=2), arch.wavlm_init_state),
                                   ("w2vbert", native.Wav2Vec2Bert, dict(arch.W2V_BERT_DIMS, n_layer=2), arch.w2vbert_init_state)):
            st = init(d, 0)
            e = cls(d, st)
            size(f"lds_{name}_workspace_bytes", e.h, 3, 16000)
            size(f"lds_{name}_workspace_bytes", e.h, 16, 480000)
            creates(name, lambda s: cls(d, s), st, last_1d(st))
            del e
        st = arch.whisper_init_state(128, 128, 2, 0)
        mkw = lambda s: native.Whisper(128, 128, 2, 2, 1500, s, arch.whisper_mel_filters(128))      # noqa: E731
        wh = mkw(st)
        size("lds_whisper_workspace_bytes", wh.h, 3, 16000)
        size("lds_whisper_workspace_bytes", wh.h, 16, 480000)
        creates("whisper", mkw, st, last_1d(st))

    for section in (lm, llama, xvector, plans, unet, encoders):
        try:
            section()
        except Exception as e:      # noqa: BLE001 -- reported; whatever it was, nothing more is launched
            DOC["errors"] = {section.__name__: repr(e)}
            break


def main():
    global L
    try:      # torch first: the library then shares the HIP runtime torch has initialised, as it does in the tests
        import torch
        DOC["gpu"] = torch.cuda.is_available()
        if DOC["gpu"]:
            torch.zeros(1, device="cuda")
    except ImportError:
        DOC["gpu"] = False
    native.LIB_PATH = os.path.abspath(sys.argv[1])
    L = native.lib()
    handle_free()
    if DOC["gpu"]:
        with_gpu()
    print(json.dumps(DOC, indent=1, sort_keys=True, default=repr))


if __name__ == "__main__":
    main()
