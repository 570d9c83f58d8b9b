"""Architecture enumeration for the hot path: parameter names and shapes.

The denoiser is the reference's ``UNet1DConditionModel`` as configured by
``Unit2Mel`` (reference diffusion/unit2mel.py:62-71): four down blocks
(3x CrossAttnDown + Down), a cross-attn mid block, four up blocks
(Up + 3x CrossAttnUp), ``layers_per_block`` resnets per down block (+1 per up
block), 8 GroupNorm groups, 8 attention heads, scale/shift time conditioning.
Key names follow the reference modules' ``state_dict`` (reference
diffusion/unet1d/unet_1d_condition.py:151-607, unet_1d_blocks.py:861-1096,
1985-2206, resnet.py:461-589, transformer_1d.py:41-224, attention.py:26-128)
so that a reference checkpoint's ``ckpt['model']`` loads unchanged.

The vocoder decoder is the reference's HiFi-VAEGAN ``Generator`` (reference
encoder/hifi_vaegan/modules/models.py:224-247) whose checkpoint carries
weight-norm pairs ``weight_g`` / ``weight_v``.

tests/golden/manifest_*.json hold the key->shape lists captured from the
reference modules; tests/test_arch.py checks this enumeration against them.
"""
from collections import OrderedDict

TIME_EMBED_DIM_MULT = 4


def unet_config(out_dims=80, n_hidden=256, block_out_channels=(256, 384, 512, 512),
                n_layers=2, n_heads=8, norm_groups=8):
    boc = tuple(int(c) for c in block_out_channels)
    return dict(
        in_channels=out_dims + n_hidden, out_channels=out_dims, x_channels=out_dims,
        cond_channels=n_hidden, block_out_channels=boc, layers_per_block=int(n_layers),
        heads=int(n_heads), groups=int(norm_groups), time_embed_dim=boc[0] * TIME_EMBED_DIM_MULT,
        time_proj_dim=boc[0])


def _resnet(d, p, cin, cout, temb):
    d[p + "norm1.weight"] = (cin,)
    d[p + "norm1.bias"] = (cin,)
    d[p + "conv1.weight"] = (cout, cin, 3)
    d[p + "conv1.bias"] = (cout,)
    d[p + "time_emb_proj.weight"] = (2 * cout, temb)
    d[p + "time_emb_proj.bias"] = (2 * cout,)
    d[p + "norm2.weight"] = (cout,)
    d[p + "norm2.bias"] = (cout,)
    d[p + "conv2.weight"] = (cout, cout, 3)
    d[p + "conv2.bias"] = (cout,)
    if cin != cout:
        d[p + "conv_shortcut.weight"] = (cout, cin, 1)
        d[p + "conv_shortcut.bias"] = (cout,)


def _transformer(d, p, c):
    d[p + "norm.weight"] = (c,)
    d[p + "norm.bias"] = (c,)
    d[p + "proj_in.weight"] = (c, c, 1)
    d[p + "proj_in.bias"] = (c,)
    b = p + "transformer_blocks.0."
    for i in (1, 2):
        d[b + f"norm{i}.weight"] = (c,)
        d[b + f"norm{i}.bias"] = (c,)
        d[b + f"attn{i}.to_q.weight"] = (c, c)
        d[b + f"attn{i}.to_k.weight"] = (c, c)
        d[b + f"attn{i}.to_v.weight"] = (c, c)
        d[b + f"attn{i}.to_out.0.weight"] = (c, c)
        d[b + f"attn{i}.to_out.0.bias"] = (c,)
    d[b + "norm3.weight"] = (c,)
    d[b + "norm3.bias"] = (c,)
    d[b + "ff.net.0.proj.weight"] = (8 * c, c)
    d[b + "ff.net.0.proj.bias"] = (8 * c,)
    d[b + "ff.net.2.weight"] = (c, 4 * c)
    d[b + "ff.net.2.bias"] = (c,)
    d[p + "proj_out.weight"] = (c, c, 1)
    d[p + "proj_out.bias"] = (c,)


def unet_blocks(cfg):
    """Structural description shared by the parameter enumeration, the numpy
    oracle and the native plan builder: a list of dicts in execution order."""
    boc = cfg["block_out_channels"]
    L = cfg["layers_per_block"]
    nb = len(boc)
    down = []
    skip_ch = [boc[0]]
    cout = boc[0]
    for i, c in enumerate(boc):
        cin, cout = cout, c
        last = i == nb - 1
        res = [(cin if j == 0 else cout, cout) for j in range(L)]
        down.append(dict(kind="down", idx=i, attn=not last, resnets=res, downsample=not last, ch=cout))
        skip_ch += [cout] * L
        if not last:
            skip_ch.append(cout)
    mid = dict(kind="mid", ch=boc[-1])
    rev = list(reversed(boc))
    up = []
    stack = list(skip_ch)
    cout = rev[0]
    for i, c in enumerate(rev):
        prev = cout
        cout = c
        last = i == nb - 1
        res = []
        for j in range(L + 1):
            sk = stack.pop()
            hin = prev if j == 0 else cout
            res.append((hin, sk, cout))  # (hidden in, skip in, out)
        up.append(dict(kind="up", idx=i, attn=i != 0, resnets=res, upsample=not last, ch=cout))
    return down, mid, up


def unet_param_shapes(cfg):
    d = OrderedDict()
    boc = cfg["block_out_channels"]
    temb = cfg["time_embed_dim"]
    d["conv_in.weight"] = (boc[0], cfg["in_channels"], 3)
    d["conv_in.bias"] = (boc[0],)
    d["time_embedding.linear_1.weight"] = (temb, cfg["time_proj_dim"])
    d["time_embedding.linear_1.bias"] = (temb,)
    d["time_embedding.linear_2.weight"] = (temb, temb)
    d["time_embedding.linear_2.bias"] = (temb,)
    down, mid, up = unet_blocks(cfg)
    for blk in down:
        p = f"down_blocks.{blk['idx']}."
        if blk["attn"]:
            for j in range(len(blk["resnets"])):
                _transformer(d, p + f"attentions.{j}.", blk["ch"])
        for j, (cin, cout) in enumerate(blk["resnets"]):
            _resnet(d, p + f"resnets.{j}.", cin, cout, temb)
        if blk["downsample"]:
            d[p + "downsamplers.0.conv.weight"] = (blk["ch"], blk["ch"], 3)
            d[p + "downsamplers.0.conv.bias"] = (blk["ch"],)
    for blk in up:
        p = f"up_blocks.{blk['idx']}."
        if blk["attn"]:
            for j in range(len(blk["resnets"])):
                _transformer(d, p + f"attentions.{j}.", blk["ch"])
        for j, (hin, sk, cout) in enumerate(blk["resnets"]):
            _resnet(d, p + f"resnets.{j}.", hin + sk, cout, temb)
        if blk["upsample"]:
            d[p + "upsamplers.0.conv.weight"] = (blk["ch"], blk["ch"], 3)
            d[p + "upsamplers.0.conv.bias"] = (blk["ch"],)
    c = mid["ch"]
    _transformer(d, "mid_block.attentions.0.", c)
    _resnet(d, "mid_block.resnets.0.", c, c, temb)
    _resnet(d, "mid_block.resnets.1.", c, c, temb)
    d["conv_norm_out.weight"] = (boc[0],)
    d["conv_norm_out.bias"] = (boc[0],)
    d["conv_out.weight"] = (cfg["out_channels"], boc[0], 3)
    d["conv_out.bias"] = (cfg["out_channels"],)
    return d


DIFFUSION_BUFFERS = (
    "betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod",
    "sqrt_one_minus_alphas_cumprod", "log_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod",
    "sqrt_recipm1_alphas_cumprod", "posterior_variance", "posterior_log_variance_clipped",
    "posterior_mean_coef1", "posterior_mean_coef2")


def unit2mel_param_shapes(input_channel, n_spk, cfg, timesteps=1000):
    """Full ``Unit2Mel.state_dict()`` key->shape (reference diffusion/unit2mel.py:52-71,
    diffusion/diffusion.py:64-85)."""
    d = OrderedDict()
    nh = cfg["cond_channels"]
    d["unit_embed.weight"] = (nh, input_channel)
    d["unit_embed.bias"] = (nh,)
    if n_spk is not None and n_spk > 1:
        d["spk_embed.weight"] = (n_spk, nh)
    for b in DIFFUSION_BUFFERS:
        d["decoder." + b] = (timesteps,)
    d["decoder.spec_min"] = (1, 1, 1)
    d["decoder.spec_max"] = (1, 1, 1)
    for k, s in unet_param_shapes(cfg).items():
        d["decoder.denoise_fn." + k] = s
    return d


# Synthetic HiFi-GAN-V1-shaped vocoder config (the real one lives only in
# the absent checkpoint pretrain/hifi-vaegan/decoder.pth["config"]).
SYNTHETIC_VOCODER_H = dict(
    sampling_rate=44100, hop_size=512, inter_channels=80, resblock="1",
    resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]],
    upsample_rates=[8, 8, 2, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4, 4],
    upsample_initial_channel=512)


def generator_param_shapes(h):
    """``Generator.state_dict()`` before remove_weight_norm (reference
    encoder/hifi_vaegan/modules/models.py:224-247, 161-222)."""
    d = OrderedDict()

    def wn(p, wshape, nbias):
        d[p + "bias"] = (nbias,)
        d[p + "weight_g"] = (wshape[0], 1, 1)
        d[p + "weight_v"] = tuple(wshape)

    c0 = h["upsample_initial_channel"]
    wn("conv_pre.", (c0, h["inter_channels"], 7), c0)
    for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
        wn(f"ups.{i}.", (c0 // 2 ** i, c0 // 2 ** (i + 1), k), c0 // 2 ** (i + 1))
    nk = len(h["resblock_kernel_sizes"])
    ch = c0
    for i in range(len(h["upsample_rates"])):
        ch = c0 // 2 ** (i + 1)
        for j, (k, dil) in enumerate(zip(h["resblock_kernel_sizes"], h["resblock_dilation_sizes"])):
            p = f"resblocks.{i * nk + j}."
            if h["resblock"] == "1":
                for m in range(len(dil)):
                    wn(p + f"convs1.{m}.", (ch, ch, k), ch)
                for m in range(len(dil)):
                    wn(p + f"convs2.{m}.", (ch, ch, k), ch)
            else:
                for m in range(len(dil)):
                    wn(p + f"convs.{m}.", (ch, ch, k), ch)
    wn("conv_post.", (1, ch, 7), 1)
    return d


def encoder_param_shapes(h):
    """``Encoder.state_dict()`` before remove_weight_norm (reference encoder/hifi_vaegan/modules/models.py:14-37): the
    generator's stages in reverse, with Conv1d downsamplers ([Cout][Cin][k], so weight_g is per output channel)."""
    d = OrderedDict()

    def wn(p, wshape, nbias):
        d[p + "bias"] = (nbias,)
        d[p + "weight_g"] = (wshape[0], 1, 1)
        d[p + "weight_v"] = tuple(wshape)

    c0, n = h["upsample_initial_channel"], len(h["upsample_rates"])
    wn("conv_pre.", (c0 // 2 ** n, 1, 7), c0 // 2 ** n)
    for i, k in enumerate(reversed(h["upsample_kernel_sizes"])):
        cin, cout = c0 // 2 ** (n - i), c0 // 2 ** (n - i - 1)
        wn(f"ups.{i}.", (cout, cin, k), cout)
    nk = len(h["resblock_kernel_sizes"])
    ch = c0
    for i in range(n):
        ch = c0 // 2 ** (n - 1 - i)
        for j, (k, dil) in enumerate(zip(h["resblock_kernel_sizes"], h["resblock_dilation_sizes"])):
            p = f"resblocks.{i * nk + j}."
            if h["resblock"] == "1":
                for m in range(len(dil)):
                    wn(p + f"convs1.{m}.", (ch, ch, k), ch)
                for m in range(len(dil)):
                    wn(p + f"convs2.{m}.", (ch, ch, k), ch)
            else:
                for m in range(len(dil)):
                    wn(p + f"convs.{m}.", (ch, ch, k), ch)
    wn("conv_post.", (2 * h["inter_channels"], ch, 7), 2 * h["inter_channels"])
    return d


def get_encoder_out_channels(encoder):
    """Reference tools/tools.py:257-264 (`get_encdoer_out_channels`)."""
    table = {"whisper_large_v3": 1280, "contentvec768l12": 768, "xlsr_53_56k": 1024, "hubertsoft": 256, "wavlmbase+": 768, "wavlmlarge": 1024}
    if encoder in table:
        return table[encoder]
    raise ValueError(f"[x] Unknown encoder: {encoder}")


# ---- text2semantic RoFormer (reference text2semantic/roformer/roformer.py:8-160; HF transformers RoFormerModel /
# RoFormerForCausalLM): phone-mode encoder (4 layers) + causal decoder with cross-attention (1 layer) --------------------
PHONE_SYMBOLS = 108      # len(symbols) in reference text/symbols.py:1-33 (pad + sorted phone set + punctuation)
NUM_TONES = 11           # reference text/symbols.py:36 (6 zh + 1 ja + 4 en)


def roformer_config(n_spk=323, semantic_kmeans_num=4096, hidden_size=256, num_attention_heads=8, intermediate_size=512,
                    encoder_layers=4, decoder_layers=1, max_position_embeddings=3072, layer_norm_eps=1e-12):
    """Shapes of `get_model(n_spk, **config['text2semantic'])` in phone mode (reference configs/config.yaml:56-83)."""
    return dict(n_spk=n_spk, semantic_kmeans_num=semantic_kmeans_num, hidden=hidden_size, heads=num_attention_heads,
                inter=intermediate_size, enc_layers=encoder_layers, dec_layers=decoder_layers, max_pos=max_position_embeddings,
                eps=float(layer_norm_eps), text_vocab=PHONE_SYMBOLS + 3, type_vocab=NUM_TONES + 1,
                text_bos=PHONE_SYMBOLS, text_eos=PHONE_SYMBOLS + 1, text_pad=PHONE_SYMBOLS + 2,
                sem_vocab=semantic_kmeans_num + 3, sem_bos=semantic_kmeans_num, sem_eos=semantic_kmeans_num + 1,
                sem_pad=semantic_kmeans_num + 2)


def _roformer_attention(d, p, h):
    for n in ("query", "key", "value"):
        d[p + f"self.{n}.weight"] = (h, h)
        d[p + f"self.{n}.bias"] = (h,)
    d[p + "output.dense.weight"] = (h, h)
    d[p + "output.dense.bias"] = (h,)
    d[p + "output.LayerNorm.weight"] = (h,)
    d[p + "output.LayerNorm.bias"] = (h,)


def _roformer_stack(d, p, cfg, vocab, type_vocab, layers, cross):
    h, it = cfg["hidden"], cfg["inter"]
    d[p + "embeddings.word_embeddings.weight"] = (vocab, h)
    d[p + "embeddings.token_type_embeddings.weight"] = (type_vocab, h)
    d[p + "embeddings.LayerNorm.weight"] = (h,)
    d[p + "embeddings.LayerNorm.bias"] = (h,)
    d[p + "encoder.embed_positions.weight"] = (cfg["max_pos"], h // cfg["heads"])
    for i in range(layers):
        q = p + f"encoder.layer.{i}."
        _roformer_attention(d, q + "attention.", h)
        if cross:
            _roformer_attention(d, q + "crossattention.", h)
        d[q + "intermediate.dense.weight"] = (it, h)
        d[q + "intermediate.dense.bias"] = (it,)
        d[q + "output.dense.weight"] = (h, it)
        d[q + "output.dense.bias"] = (h,)
        d[q + "output.LayerNorm.weight"] = (h,)
        d[q + "output.LayerNorm.bias"] = (h,)


def roformer_param_shapes(cfg):
    """`Roformer.state_dict()` key -> shape (reference roformer.py:59-125 over HF RoFormerModel / RoFormerForCausalLM).
    `*.embed_positions.weight` is the fixed sinusoid table, `cls.predictions.decoder.{weight,bias}` are tied to the word
    embeddings / `cls.predictions.bias`."""
    d = OrderedDict()
    h = cfg["hidden"]
    _roformer_stack(d, "text_encoder.", cfg, cfg["text_vocab"], cfg["type_vocab"], cfg["enc_layers"], False)
    _roformer_stack(d, "semantic_decoder.roformer.", cfg, cfg["sem_vocab"], 1, cfg["dec_layers"], True)
    d["semantic_decoder.cls.predictions.bias"] = (cfg["sem_vocab"],)
    d["semantic_decoder.cls.predictions.transform.dense.weight"] = (h, h)
    d["semantic_decoder.cls.predictions.transform.dense.bias"] = (h,)
    d["semantic_decoder.cls.predictions.transform.LayerNorm.weight"] = (h,)
    d["semantic_decoder.cls.predictions.transform.LayerNorm.bias"] = (h,)
    d["semantic_decoder.cls.predictions.decoder.weight"] = (cfg["sem_vocab"], h)
    d["semantic_decoder.cls.predictions.decoder.bias"] = (cfg["sem_vocab"],)
    if cfg["n_spk"] is not None and cfg["n_spk"] > 1:
        d["spk_emb.weight"] = (cfg["n_spk"] + 1, h)
    return d


ROFORMER_TIED = {"semantic_decoder.cls.predictions.decoder.weight": "semantic_decoder.roformer.embeddings.word_embeddings.weight",
                 "semantic_decoder.cls.predictions.decoder.bias": "semantic_decoder.cls.predictions.bias"}


def roformer_sinusoid_table(n_pos, dim):
    """HF RoFormerSinusoidalPositionalEmbedding.create_weight: [sin(pos * w_i) | cos(pos * w_i)], w_i = 10000^(-2i/dim),
    evaluated in float64 and rounded to fp32 once."""
    import numpy as np
    pos = np.arange(n_pos, dtype=np.float64)[:, None]
    inv = 1.0 / np.power(10000.0, 2.0 * np.arange(dim // 2, dtype=np.float64) / dim)
    ang = pos * inv[None, :]
    return np.concatenate([np.sin(ang), np.cos(ang)], axis=1).astype(np.float32)


def roformer_init_state(cfg, seed=0, init_weights=None):
    """Build-owned seeded weights for the LM (no checkpoint ships): per-key integer RNG, tied tensors made identical, the
    position tables computed.  `init_weights` = the lds.init_weights module when this file is loaded outside the package."""
    if init_weights is None:
        from . import init_weights
    import numpy as np
    shapes = roformer_param_shapes(cfg)
    st = init_weights.init_state(shapes, seed)
    for k in shapes:
        if k.endswith("embed_positions.weight"):
            st[k] = roformer_sinusoid_table(*shapes[k])
        elif "LayerNorm.weight" in k:
            st[k] = init_weights.uniform(k, shapes[k], seed, 0.8, 1.2)
        elif "embeddings.weight" in k or k == "spk_emb.weight":
            st[k] = init_weights.uniform(k, shapes[k], seed, -1.0, 1.0)
    for dst, src in ROFORMER_TIED.items():
        st[dst] = st[src]
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in st.items()}


# ---- text2semantic Llama (reference text2semantic/llama/llama.py:23-71 over HF LlamaForCausalLM): one decoder-only stack over the stream
# [phone BOS, phones, phone EOS, semantic BOS, semantic tokens ...] ------------------------------------------------------------------------
def llama_config(semantic_kmeans_num=10000, hidden_size=4096, num_attention_heads=32, num_key_value_heads=None, head_dim=None,
                 intermediate_size=11008, num_hidden_layers=32, max_position_embeddings=2048, rms_norm_eps=1e-6, rope_theta=10000.0):
    """Shapes and ids of `Llama(config, mode="phone", semantic_kmeans_num=K)` (defaults: HF LlamaConfig's).  The phone-side BOS / EOS / PAD
    (108, 109, 110) coincide with the shifted semantic ids 0, 1, 2: that is the reference's numbering (llama.py:39-58)."""
    kv = num_attention_heads if num_key_value_heads is None else num_key_value_heads
    d = hidden_size // num_attention_heads if head_dim is None else head_dim
    s, K = PHONE_SYMBOLS, semantic_kmeans_num
    return dict(semantic_kmeans_num=K, hidden=hidden_size, heads=num_attention_heads, kv_heads=kv, head_dim=d, inter=intermediate_size,
                layers=num_hidden_layers, max_pos=max_position_embeddings, eps=float(rms_norm_eps), rope_theta=float(rope_theta),
                text_bos=s, text_eos=s + 1, text_pad=s + 2, shift=s, bos=s + K, eos=s + K + 1, pad=s + K + 2, vocab=s + K + 3)


def llama_param_shapes(cfg):
    """`Llama.state_dict()` key -> shape (llama.py:65; tie_word_embeddings is False there, so lm_head.weight is a tensor of its own)"""
    d = OrderedDict()
    h, qd, kd, it = cfg["hidden"], cfg["heads"] * cfg["head_dim"], cfg["kv_heads"] * cfg["head_dim"], cfg["inter"]
    d["llama.model.embed_tokens.weight"] = (cfg["vocab"], h)
    for i in range(cfg["layers"]):
        p = f"llama.model.layers.{i}."
        d[p + "self_attn.q_proj.weight"] = (qd, h)
        d[p + "self_attn.k_proj.weight"] = (kd, h)
        d[p + "self_attn.v_proj.weight"] = (kd, h)
        d[p + "self_attn.o_proj.weight"] = (h, qd)
        d[p + "mlp.gate_proj.weight"] = (it, h)
        d[p + "mlp.up_proj.weight"] = (it, h)
        d[p + "mlp.down_proj.weight"] = (h, it)
        d[p + "input_layernorm.weight"] = (h,)
        d[p + "post_attention_layernorm.weight"] = (h,)
    d["llama.model.norm.weight"] = (h,)
    d["llama.lm_head.weight"] = (cfg["vocab"], h)
    return d


def llama_init_state(cfg, seed=0, init_weights=None):
    """Build-owned seeded weights for the Llama LM: matrices at the familiar 1/sqrt(fan_in) scale, norm gains around 1, unit-range embeddings"""
    if init_weights is None:
        from . import init_weights
    import numpy as np
    shapes = llama_param_shapes(cfg)
    st = init_weights.init_state(shapes, seed)
    for k in shapes:
        if k.endswith("layernorm.weight") or k.endswith("model.norm.weight"):
            st[k] = init_weights.uniform(k, shapes[k], seed, 0.8, 1.2)
        elif k.endswith("embed_tokens.weight"):
            st[k] = init_weights.uniform(k, shapes[k], seed, -1.0, 1.0)
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in st.items()}


# ---- Whisper units encoder (reference encoder/whisper/model.py:10-21,112-137; tools/tools.py:105-116) ----------------------------------
# dims of the reference's configured encoder (configs/config.yaml: whisper_large_v3); the text-side fields describe the decoder the
# reference's Whisper(dims) never builds and are carried only because ModelDimensions has them
WHISPER_LARGE_V3_DIMS = dict(n_mels=128, n_audio_ctx=1500, n_audio_state=1280, n_audio_head=20, n_audio_layer=32, n_vocab=51866,
                             n_text_ctx=448, n_text_state=1280, n_text_head=20, n_text_layer=32)


def whisper_param_shapes(n_mels, n_audio_state, n_audio_layer):
    """`Whisper(dims).state_dict()` key -> shape: the audio encoder only (`key` has no bias, model.py:47)"""
    d = OrderedDict()
    c = int(n_audio_state)
    d["encoder.conv1.weight"] = (c, int(n_mels), 3)
    d["encoder.conv1.bias"] = (c,)
    d["encoder.conv2.weight"] = (c, c, 3)
    d["encoder.conv2.bias"] = (c,)
    for i in range(int(n_audio_layer)):
        p = f"encoder.blocks.{i}."
        d[p + "attn.query.weight"] = (c, c)
        d[p + "attn.query.bias"] = (c,)
        d[p + "attn.key.weight"] = (c, c)
        d[p + "attn.value.weight"] = (c, c)
        d[p + "attn.value.bias"] = (c,)
        d[p + "attn.out.weight"] = (c, c)
        d[p + "attn.out.bias"] = (c,)
        d[p + "attn_ln.weight"] = (c,)
        d[p + "attn_ln.bias"] = (c,)
        d[p + "mlp.0.weight"] = (4 * c, c)
        d[p + "mlp.0.bias"] = (4 * c,)
        d[p + "mlp.2.weight"] = (c, 4 * c)
        d[p + "mlp.2.bias"] = (c,)
        d[p + "mlp_ln.weight"] = (c,)
        d[p + "mlp_ln.bias"] = (c,)
    d["encoder.ln_post.weight"] = (c,)
    d["encoder.ln_post.bias"] = (c,)
    return d


def whisper_init_state(n_mels, n_audio_state, n_audio_layer, seed=0, init_weights=None):
    """Build-owned seeded weights for the units encoder (no checkpoint ships): LayerNorm gains in [0.8, 1.2), LayerNorm biases in
    [-0.1, 0.1), everything else by lds.init_weights' role rules.  `init_weights` = that module when this file is loaded by path."""
    if init_weights is None:
        from . import init_weights
    import numpy as np
    shapes = whisper_param_shapes(n_mels, n_audio_state, n_audio_layer)
    st = init_weights.init_state(shapes, seed)
    for k in shapes:
        if "_ln." in k or ".ln_post." in k:
            st[k] = init_weights.uniform(k, shapes[k], seed, 0.8, 1.2) if k.endswith(".weight") else init_weights.uniform(k, shapes[k], seed, -0.1, 0.1)
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in st.items()}


# ---- Whisper text decoder (OpenAI whisper/model.py TextDecoder; the reference's model.py:85-110 holds its blocks) -----------------------
def whisper_decoder_param_shapes(n_vocab, n_text_ctx, n_text_state, n_text_layer):
    """OpenAI's `decoder.*` state_dict key -> shape, in the module order of TextDecoder (`key` has no bias)"""
    d = OrderedDict()
    c = int(n_text_state)
    d["decoder.positional_embedding"] = (int(n_text_ctx), c)
    d["decoder.token_embedding.weight"] = (int(n_vocab), c)
    for i in range(int(n_text_layer)):
        p = f"decoder.blocks.{i}."
        for a in ("attn", "cross_attn"):
            d[p + a + ".query.weight"] = (c, c)
            d[p + a + ".query.bias"] = (c,)
            d[p + a + ".key.weight"] = (c, c)
            d[p + a + ".value.weight"] = (c, c)
            d[p + a + ".value.bias"] = (c,)
            d[p + a + ".out.weight"] = (c, c)
            d[p + a + ".out.bias"] = (c,)
            d[p + a + "_ln.weight"] = (c,)
            d[p + a + "_ln.bias"] = (c,)
        d[p + "mlp.0.weight"] = (4 * c, c)
        d[p + "mlp.0.bias"] = (4 * c,)
        d[p + "mlp.2.weight"] = (c, 4 * c)
        d[p + "mlp.2.bias"] = (c,)
        d[p + "mlp_ln.weight"] = (c,)
        d[p + "mlp_ln.bias"] = (c,)
    d["decoder.ln.weight"] = (c,)
    d["decoder.ln.bias"] = (c,)
    return d


def whisper_decoder_init_state(n_vocab, n_text_ctx, n_text_state, n_text_layer, seed=0, init_weights=None):
    """Build-owned seeded weights for the text decoder.  Matrices at 3x the familiar 1/sqrt(fan_in) scale and unit-range embeddings: the
    blocks then move the residual stream enough, and the tied head spreads the logits enough, that a seeded greedy path is not razor-thin
    (the fixture recipe records every path's smallest top-2 gap and refuses a seed below 1e-3 x absmax)."""
    if init_weights is None:
        from . import init_weights
    import numpy as np
    shapes = whisper_decoder_param_shapes(n_vocab, n_text_ctx, n_text_state, n_text_layer)
    st = {}
    for k, sh in shapes.items():
        if "_ln." in k or ".ln." in k:
            st[k] = init_weights.uniform(k, sh, seed, 0.8, 1.2) if k.endswith(".weight") else init_weights.uniform(k, sh, seed, -0.1, 0.1)
        elif k.endswith("embedding.weight") or k.endswith("positional_embedding"):
            st[k] = init_weights.uniform(k, sh, seed, -1.0, 1.0)
        elif k.endswith(".bias"):
            st[k] = init_weights.uniform(k, sh, seed, -0.05, 0.05)
        else:
            b = 3.0 / float(np.sqrt(sh[1]))
            st[k] = init_weights.uniform(k, sh, seed, -b, b)
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in st.items()}


# openai-whisper's tokenizer.LANGUAGES in its order (the language tokens follow <|startoftranscript|> in this order); large-v3 added "yue"
WHISPER_LANGUAGES = ("en zh de es ru ko fr ja pt tr pl ca nl ar sv it id hi fi vi he uk el ms cs ro da hu ta no th ur hr bg lt la mi ml cy sk te fa lv bn "
                     "sr az sl kn et mk br eu is hy ne mn bs kk sq sw gl mr pa si km sn yo so af oc ka be tg sd gu am yi lo uz fo ht ps tk nn mt sa lb my "
                     "bo tl mg as tt haw ln ha ba jw su yue").split()


def whisper_special_tokens(n_vocab, **override):
    """The special-token ids of a multilingual Whisper vocabulary, derived as openai-whisper's get_encoding lays them out behind the 50,257
    byte-pair tokens: <|endoftext|>, <|startoftranscript|>, the n_vocab - 51766 language tokens, <|translate|>, <|transcribe|>,
    <|startoflm|>, <|startofprev|>, <|nospeech|>, <|notimestamps|>, then the 1501 timestamps <|0.00|> .. <|30.00|>.
    UNVERIFIED: written from memory of openai-whisper, with no tokenizer file at hand to confirm it against (for 51,866 it gives eot 50257,
    sot 50258, languages from 50259, translate 50359, transcribe 50360, startoflm 50361, startofprev 50362, nospeech 50363, notimestamps
    50364, timestamps from 50365).  Every id can be overridden by keyword; check them against the tokenizer that came with the checkpoint.
    Returns a dict: eot, sot, translate, transcribe, startoflm, startofprev, nospeech, notimestamps, timestamp_begin, num_languages,
    languages (code -> id)."""
    n_vocab = int(n_vocab)
    if n_vocab < 51865:
        raise ValueError(f"whisper_special_tokens derives multilingual vocabularies (n_vocab >= 51865); for {n_vocab} pass every id yourself")
    nl = n_vocab - 51765 - 1
    if nl > len(WHISPER_LANGUAGES):
        raise ValueError(f"n_vocab {n_vocab} implies {nl} languages; the table knows {len(WHISPER_LANGUAGES)}")
    eot = 50257
    t = dict(eot=eot, sot=eot + 1, translate=eot + 2 + nl, transcribe=eot + 3 + nl, startoflm=eot + 4 + nl, startofprev=eot + 5 + nl,
             nospeech=eot + 6 + nl, notimestamps=eot + 7 + nl, timestamp_begin=eot + 8 + nl, num_languages=nl)
    t["languages"] = {code: eot + 2 + i for i, code in enumerate(WHISPER_LANGUAGES[:nl])}
    unknown = set(override) - set(t)
    if unknown:
        raise TypeError(f"unknown special token(s) {sorted(unknown)}")
    t.update(override)
    return t


def whisper_mel_filters(n_mels, sr=16000, n_fft=400):
    """The filter bank of the reference's assets/mel_filters.npz ([n_mels][201], float32), computed: librosa.filters.mel(sr=16000,
    n_fft=400, n_mels=n_mels) -- Slaney's scale (linear below 1 kHz, logarithmic above), triangles normalised to unit area -- evaluated
    in float64 and rounded once."""
    import numpy as np
    assert n_mels in (80, 128), f"Unsupported n_mels: {n_mels}"
    fftfreqs = np.linspace(0.0, sr / 2.0, 1 + n_fft // 2)
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0

    def hz_to_mel(f):
        return f / f_sp if f < min_log_hz else min_log_mel + np.log(f / min_log_hz) / logstep

    mels = np.linspace(hz_to_mel(0.0), hz_to_mel(sr / 2.0), n_mels + 2)
    mel_f = np.where(mels >= min_log_mel, min_log_hz * np.exp(logstep * (mels - min_log_mel)), f_sp * mels)
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fftfreqs[None, :]
    w = np.zeros((n_mels, 1 + n_fft // 2))
    for i in range(n_mels):
        w[i] = np.maximum(0.0, np.minimum(-ramps[i] / fdiff[i], ramps[i + 2] / fdiff[i + 1]))
    w *= (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]
    return w.astype(np.float32)


# ---- HuBERT units encoder (reference encoder/hubert/model.py:19-148: HuBERT-base; HuBERT-Soft and ContentVec are this network) ----------
# the fields of include/lds.h lds_hubert_cfg; n_ctx = the most frames of one call (30 s)
HUBERT_BASE_DIMS = dict(conv_dim=512, n_state=768, n_head=12, n_layer=12, n_ffn=3072, n_proj=256, pos_kernel=128, pos_groups=16, n_ctx=1500)
HUBERT_HOP, HUBERT_PAD, HUBERT_MIN_SAMPLES = 320, 40, 320      # HubertSoft.units: 40 zeros per side, then L // 320 frames


def hubert_level_frames(n_samples, pad=HUBERT_PAD):
    """Frames after conv0 .. conv6 for a clip of n_samples padded by `pad` zeros per side (model.py:99-106): conv0 k 10 stride 5,
    conv1..4 k 3 stride 2, conv5..6 k 2 stride 2, none padded."""
    n = [(int(n_samples) + 2 * pad - 10) // 5 + 1]
    for i in range(1, 7):
        n.append((n[-1] - 3) // 2 + 1 if i <= 4 else (n[-1] - 2) // 2 + 1)
    return n


def hubert_frames(n_samples, pad=HUBERT_PAD):
    """Frames the feature extractor gives for the clip (the last of hubert_level_frames).  With pad 40 this is n_samples // 320."""
    return hubert_level_frames(n_samples, pad)[-1]


def hubert_param_shapes(cfg=None, num_label_embeddings=100):
    """`Hubert(num_label_embeddings).state_dict()` key -> shape, in the reference's order (masked_spec_embed and label_embedding.weight,
    which inference never reads, included: a checkpoint loads with strict=True)"""
    c = dict(HUBERT_BASE_DIMS if cfg is None else cfg)
    D, C, F, P, K, G = c["conv_dim"], c["n_state"], c["n_ffn"], c["n_proj"], c["pos_kernel"], c["pos_groups"]
    d = OrderedDict()
    d["masked_spec_embed"] = (C,)
    d["feature_extractor.conv0.weight"] = (D, 1, 10)
    d["feature_extractor.norm0.weight"] = (D,)
    d["feature_extractor.norm0.bias"] = (D,)
    for i in range(1, 7):
        d[f"feature_extractor.conv{i}.weight"] = (D, D, 3 if i <= 4 else 2)
    d["feature_projection.norm.weight"] = (D,)
    d["feature_projection.norm.bias"] = (D,)
    d["feature_projection.projection.weight"] = (C, D)
    d["feature_projection.projection.bias"] = (C,)
    d["positional_embedding.conv.bias"] = (C,)
    d["positional_embedding.conv.parametrizations.weight.original0"] = (1, 1, K)
    d["positional_embedding.conv.parametrizations.weight.original1"] = (C, C // G, K)
    d["norm.weight"] = (C,)
    d["norm.bias"] = (C,)
    for i in range(c["n_layer"]):
        p = f"encoder.layers.{i}."
        d[p + "self_attn.in_proj_weight"] = (3 * C, C)
        d[p + "self_attn.in_proj_bias"] = (3 * C,)
        d[p + "self_attn.out_proj.weight"] = (C, C)
        d[p + "self_attn.out_proj.bias"] = (C,)
        d[p + "linear1.weight"] = (F, C)
        d[p + "linear1.bias"] = (F,)
        d[p + "linear2.weight"] = (C, F)
        d[p + "linear2.bias"] = (C,)
        d[p + "norm1.weight"] = (C,)
        d[p + "norm1.bias"] = (C,)
        d[p + "norm2.weight"] = (C,)
        d[p + "norm2.bias"] = (C,)
    d["proj.weight"] = (P, C)
    d["proj.bias"] = (P,)
    d["label_embedding.weight"] = (int(num_label_embeddings), P)
    return d


def hubert_init_state(cfg=None, seed=0, init_weights=None, num_label_embeddings=100):
    """Build-owned seeded weights (no checkpoint ships), scaled so that every stage lives at a scale of order 1 (torch's default
    initialisation leaves the convolution stack at 2e-3, where an error would hide behind the next LayerNorm): the feature extractor's
    GELU convolutions get He's bound sqrt(6 / fan_in), the positional convolution's per-tap norms g lie in [1.5, 3) (a sum over 128 taps
    of variance g^2 / 768 each), in_proj three times the default bound (attention logits of standard deviation ~3); norms and everything
    else by lds.init_weights' role rules.  `init_weights` = that module when this file is loaded by path."""
    if init_weights is None:
        from . import init_weights
    import numpy as np
    shapes = hubert_param_shapes(cfg, num_label_embeddings)
    st = init_weights.init_state(shapes, seed)
    for k, shp in shapes.items():
        fan = int(np.prod(shp[1:])) if len(shp) > 1 else 1
        if k.startswith("feature_extractor.conv"):
            b = float(np.sqrt(6.0 / fan))
            st[k] = init_weights.uniform(k, shp, seed, -b, b)
        elif k.endswith("weight.original0"):
            st[k] = init_weights.uniform(k, shp, seed, 1.5, 3.0)
        elif k.endswith("in_proj_weight"):
            b = float(3.0 / np.sqrt(fan))
            st[k] = init_weights.uniform(k, shp, seed, -b, b)
        elif k == "norm.weight":      # (the role rules know a norm by the dot in front of its name)
            st[k] = init_weights.uniform(k, shp, seed, 0.8, 1.2)
        elif k == "norm.bias":
            st[k] = init_weights.uniform(k, shp, seed, -0.1, 0.1)
        elif k == "masked_spec_embed":
            st[k] = init_weights.uniform(k, shp, seed, 0.0, 1.0)
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in st.items()}


def hubert_fold_weight_norm(g, v):
    """parametrizations.weight_norm(conv, dim=2) folded in float64: w[:, :, k] = g[k] v[:, :, k] / |v[:, :, k]|, the norm over the other
    two axes (what lds_hubert_create does at pack time)."""
    import numpy as np
    v64 = np.asarray(v, dtype=np.float64)
    n = np.sqrt((v64 * v64).sum(axis=(0, 1), keepdims=True))
    return np.asarray(g, dtype=np.float64).reshape(1, 1, -1) * v64 / n


# ---- wav2vec 2.0 units encoder, layer-norm flavour (XLSR-53: reference tools/tools.py Audio2xlsr_53_56k) ------------------------------------
# the fields of include/lds.h lds_w2v_cfg; n_ctx = the most frames of one call (30 s give 1499)
XLSR_53_DIMS = dict(conv_dim=512, n_state=1024, n_head=16, n_layer=24, n_ffn=4096, pos_kernel=128, pos_groups=16, n_ctx=1500)
W2V_MIN_SAMPLES = 400
# checkpoint tensors that inference never reads (fairseq's pre-training heads; transformers' name of mask_emb)
W2V_IGNORED_PREFIXES = ("mask_emb", "masked_spec_embed", "quantizer.", "project_q.", "final_proj.")


def w2v_frames(n_samples):
    """Frames of a clip of n_samples: HuBERT's level rule without padding (400 samples -> 1, 30 s -> 1499)"""
    return hubert_level_frames(n_samples, 0)[-1]


def w2v_param_shapes(cfg=None):
    """fairseq's Wav2Vec2Model key -> shape for the tensors inference reads (the names lds_w2v_create looks up)"""
    c = dict(XLSR_53_DIMS if cfg is None else cfg)
    D, C, F, K, G = c["conv_dim"], c["n_state"], c["n_ffn"], c["pos_kernel"], c["pos_groups"]
    d = OrderedDict()
    for i in range(7):
        p = f"feature_extractor.conv_layers.{i}."
        d[p + "0.weight"] = (D, 1 if i == 0 else D, 10 if i == 0 else (3 if i <= 4 else 2))
        d[p + "0.bias"] = (D,)
        d[p + "2.1.weight"] = (D,)
        d[p + "2.1.bias"] = (D,)
    d["layer_norm.weight"] = (D,)
    d["layer_norm.bias"] = (D,)
    d["post_extract_proj.weight"] = (C, D)
    d["post_extract_proj.bias"] = (C,)
    d["encoder.pos_conv.0.bias"] = (C,)
    d["encoder.pos_conv.0.weight_g"] = (1, 1, K)
    d["encoder.pos_conv.0.weight_v"] = (C, C // G, K)
    for l in range(c["n_layer"]):
        p = f"encoder.layers.{l}."
        for n in ("k_proj", "v_proj", "q_proj", "out_proj"):
            d[p + f"self_attn.{n}.weight"] = (C, C)
            d[p + f"self_attn.{n}.bias"] = (C,)
        d[p + "self_attn_layer_norm.weight"] = (C,)
        d[p + "self_attn_layer_norm.bias"] = (C,)
        d[p + "fc1.weight"] = (F, C)
        d[p + "fc1.bias"] = (F,)
        d[p + "fc2.weight"] = (C, F)
        d[p + "fc2.bias"] = (C,)
        d[p + "final_layer_norm.weight"] = (C,)
        d[p + "final_layer_norm.bias"] = (C,)
    d["encoder.layer_norm.weight"] = (C,)
    d["encoder.layer_norm.bias"] = (C,)
    return d


def w2v_key_to_transformers(k):
    """fairseq name -> transformers.Wav2Vec2Model's state-dict name (one to one on w2v_param_shapes' keys and on mask_emb)"""
    import re
    m = re.match(r"feature_extractor\.conv_layers\.(\d+)\.(0|2\.1)\.(weight|bias)$", k)
    if m:
        return f"feature_extractor.conv_layers.{m.group(1)}.{'conv' if m.group(2) == '0' else 'layer_norm'}.{m.group(3)}"
    if k == "mask_emb":
        return "masked_spec_embed"
    for a, b in (("layer_norm.", "feature_projection.layer_norm."), ("post_extract_proj.", "feature_projection.projection.")):
        if k.startswith(a):
            return b + k[len(a):]
    fixed = {"encoder.pos_conv.0.bias": "encoder.pos_conv_embed.conv.bias",
             "encoder.pos_conv.0.weight_g": "encoder.pos_conv_embed.conv.parametrizations.weight.original0",
             "encoder.pos_conv.0.weight_v": "encoder.pos_conv_embed.conv.parametrizations.weight.original1"}
    if k in fixed:
        return fixed[k]
    m = re.match(r"(encoder\.layers\.\d+\.)(.+)$", k)
    if m:
        rest = m.group(2)
        for a, b in (("self_attn_layer_norm.", "layer_norm."), ("self_attn.", "attention."), ("fc1.", "feed_forward.intermediate_dense."),
                     ("fc2.", "feed_forward.output_dense.")):
            if rest.startswith(a):
                return m.group(1) + b + rest[len(a):]
        return k      # final_layer_norm keeps its name
    return k          # encoder.layer_norm.*


def w2v_keys_from_transformers(cfg=None):
    """transformers name -> fairseq name, for every tensor of w2v_param_shapes(cfg) and masked_spec_embed"""
    table = {w2v_key_to_transformers(k): k for k in w2v_param_shapes(cfg)}
    table["masked_spec_embed"] = "mask_emb"
    return table


def w2v_init_state(cfg=None, seed=0, init_weights=None):
    """Build-owned seeded weights in fairseq's names (no checkpoint ships), every stage at a scale of order 1 as in hubert_init_state, so
    that no error hides behind the next LayerNorm: the feature extractor's convolutions get He's bound sqrt(6 / fan_in), the positional
    convolution's per-tap norms g lie in [1.5, 3), q_proj and k_proj 1.7 times the default bound (attention logits of standard deviation
    ~3); every LayerNorm gain in [0.8, 1.2) and bias in [-0.1, 0.1); the rest by lds.init_weights' role rules."""
    if init_weights is None:
        from . import init_weights
    import numpy as np
    shapes = w2v_param_shapes(cfg)
    st = init_weights.init_state(shapes, seed)
    for k, shp in shapes.items():
        fan = int(np.prod(shp[1:])) if len(shp) > 1 else 1
        if "layer_norm." in k or ".2.1." in k:
            st[k] = init_weights.uniform(k, shp, seed, 0.8, 1.2) if k.endswith(".weight") else init_weights.uniform(k, shp, seed, -0.1, 0.1)
        elif k.startswith("feature_extractor.conv_layers.") and k.endswith(".0.weight"):
            b = float(np.sqrt(6.0 / fan))
            st[k] = init_weights.uniform(k, shp, seed, -b, b)
        elif k.endswith("weight_g"):
            st[k] = init_weights.uniform(k, shp, seed, 1.5, 3.0)
        elif k.endswith("q_proj.weight") or k.endswith("k_proj.weight"):
            b = float(1.7 / np.sqrt(fan))
            st[k] = init_weights.uniform(k, shp, seed, -b, b)
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in st.items()}


def w2v_convert_state(state, cfg=None):
    """A checkpoint's state dict in fairseq or transformers naming (an optional "module." / "w2v_encoder.w2v_model." / "wav2vec2." prefix
    removed, the pre-training tensors dropped) -> the tensors of w2v_param_shapes(cfg) in fairseq naming.  A missing tensor is a KeyError
    naming it; a wrong shape a ValueError."""
    shapes = w2v_param_shapes(cfg)
    back = w2v_keys_from_transformers(cfg)
    got = {}
    for k, v in state.items():
        for pre in ("module.", "w2v_encoder.w2v_model.", "wav2vec2."):
            if k.startswith(pre):
                k = k[len(pre):]
        if k.startswith(W2V_IGNORED_PREFIXES):
            continue
        k = k if k in shapes else back.get(k, k)
        if k in shapes:
            got[k] = v
    out = OrderedDict()
    for k, shp in shapes.items():
        if k not in got:
            raise KeyError(f"wav2vec 2.0 checkpoint lacks {k!r} (transformers name: {w2v_key_to_transformers(k)!r})")
        if tuple(got[k].shape) != tuple(shp):
            raise ValueError(f"wav2vec 2.0 checkpoint: {k!r} has shape {tuple(got[k].shape)}, expected {tuple(shp)}")
        out[k] = got[k]
    return out


# ---- w2v-BERT 2.0 units encoder (reference tools/tools.py Wav2Vec2Bert: transformers' Wav2Vec2BertModel on SeamlessM4TFeatureExtractor) --------
# the fields of include/lds.h lds_w2vbert_cfg (Wav2Vec2BertConfig()'s defaults); n_ctx = the most rows of one call (30 s give 1499)
W2V_BERT_DIMS = dict(n_mels=80, stride=2, n_state=1024, n_head=16, n_ffn=4096, n_layer=24, left_max=64, right_max=8, dw_kernel=31, n_ctx=1500,
                     eps=1e-5)
W2VBERT_MIN_SAMPLES = 560      # two frames: one frame makes the extractor's ddof = 1 variance 0 / 0
# checkpoint tensors that inference never reads
W2VBERT_IGNORED_PREFIXES = ("masked_spec_embed",)


def w2vbert_frames(n_samples):
    """(n, valid, rows) of a clip of n_samples at 16 kHz: n = 1 + (L - 400) // 160 frames of 400 samples, stacked in pairs into
    rows = (n + 1) // 2 rows of which valid = n // 2 are unmasked; with n odd the last row is the masked row"""
    n = 1 + (int(n_samples) - 400) // 160 if n_samples >= 400 else 0
    return n, n // 2, (n + 1) // 2


def w2vbert_param_shapes(cfg=None):
    """transformers' Wav2Vec2BertModel key -> shape for the tensors inference reads (the names lds_w2vbert_create looks up)"""
    c = dict(W2V_BERT_DIMS if cfg is None else cfg)
    Fd, C, F, K, NR = c["n_mels"] * c["stride"], c["n_state"], c["n_ffn"], c["dw_kernel"], c["left_max"] + c["right_max"] + 1
    d = OrderedDict()
    d["feature_projection.layer_norm.weight"] = (Fd,)
    d["feature_projection.layer_norm.bias"] = (Fd,)
    d["feature_projection.projection.weight"] = (C, Fd)
    d["feature_projection.projection.bias"] = (C,)
    for l in range(c["n_layer"]):
        p = f"encoder.layers.{l}."
        for ff in ("ffn1", "ffn2"):
            d[p + f"{ff}_layer_norm.weight"] = (C,)
            d[p + f"{ff}_layer_norm.bias"] = (C,)
            d[p + f"{ff}.intermediate_dense.weight"] = (F, C)
            d[p + f"{ff}.intermediate_dense.bias"] = (F,)
            d[p + f"{ff}.output_dense.weight"] = (C, F)
            d[p + f"{ff}.output_dense.bias"] = (C,)
        d[p + "self_attn_layer_norm.weight"] = (C,)
        d[p + "self_attn_layer_norm.bias"] = (C,)
        for n in ("linear_q", "linear_k", "linear_v", "linear_out"):
            d[p + f"self_attn.{n}.weight"] = (C, C)
            d[p + f"self_attn.{n}.bias"] = (C,)
        d[p + "self_attn.distance_embedding.weight"] = (NR, C // c["n_head"])
        d[p + "conv_module.layer_norm.weight"] = (C,)
        d[p + "conv_module.layer_norm.bias"] = (C,)
        d[p + "conv_module.pointwise_conv1.weight"] = (2 * C, C, 1)
        d[p + "conv_module.depthwise_conv.weight"] = (C, 1, K)
        d[p + "conv_module.depthwise_layer_norm.weight"] = (C,)
        d[p + "conv_module.depthwise_layer_norm.bias"] = (C,)
        d[p + "conv_module.pointwise_conv2.weight"] = (C, C, 1)
        d[p + "final_layer_norm.weight"] = (C,)
        d[p + "final_layer_norm.bias"] = (C,)
    return d


def w2vbert_init_state(cfg=None, seed=0, init_weights=None):
    """Build-owned seeded weights in transformers' names (no checkpoint ships), every stage at a scale of order 1 as in w2v_init_state, so that
    no error hides behind the next LayerNorm: every matrix uniform within sqrt(3 / fan_in) (unit gain), linear_q and linear_k within
    1.7 / sqrt(fan_in) and the distance embedding within 1 (attention logits of standard deviation ~1, the relative-key term about half
    of it), every LayerNorm gain in [0.8, 1.2), every bias in [-0.1, 0.1)."""
    if init_weights is None:
        from . import init_weights
    import numpy as np
    st = OrderedDict()
    for k, shp in w2vbert_param_shapes(cfg).items():
        fan = int(np.prod(shp[1:])) if len(shp) > 1 else 1
        if k.endswith(".bias"):
            st[k] = init_weights.uniform(k, shp, seed, -0.1, 0.1)
        elif "layer_norm." in k:
            st[k] = init_weights.uniform(k, shp, seed, 0.8, 1.2)
        elif k.endswith("distance_embedding.weight"):
            st[k] = init_weights.uniform(k, shp, seed, -1.0, 1.0)
        else:
            b = float((1.7 if ("linear_q." in k or "linear_k." in k) else np.sqrt(3.0)) / np.sqrt(fan))
            st[k] = init_weights.uniform(k, shp, seed, -b, b)
    return OrderedDict((k, np.ascontiguousarray(v, dtype=np.float32)) for k, v in st.items())


def w2vbert_convert_state(state, cfg=None):
    """A checkpoint's state dict in transformers naming (an optional "module." / "wav2vec2_bert." prefix removed, masked_spec_embed dropped)
    -> the tensors of w2vbert_param_shapes(cfg).  A missing tensor is a KeyError naming it; a wrong shape a ValueError."""
    shapes = w2vbert_param_shapes(cfg)
    got = {}
    for k, v in state.items():
        for pre in ("module.", "wav2vec2_bert."):
            if k.startswith(pre):
                k = k[len(pre):]
        if k.startswith(W2VBERT_IGNORED_PREFIXES):
            continue
        if k in shapes:
            got[k] = v
    out = OrderedDict()
    for k, shp in shapes.items():
        if k not in got:
            raise KeyError(f"w2v-BERT checkpoint lacks {k!r}")
        if tuple(got[k].shape) != tuple(shp):
            raise ValueError(f"w2v-BERT checkpoint: {k!r} has shape {tuple(got[k].shape)}, expected {tuple(shp)}")
        out[k] = got[k]
    return out


# ---- WavLM units encoder (transformers' WavLMModel: so-vits-svc's wavlmbase+, kNN-VC's WavLM-Large) ------------------------------------------
# the fields of include/lds.h lds_wavlm_cfg; stable_layer_norm 0 = Base / Base+ (group-norm extractor, post-LN blocks), 1 = Large (layer-norm
# extractor, pre-LN blocks); n_ctx = the most frames of one call (30 s give 1499)
WAVLM_BASE_PLUS_DIMS = dict(conv_dim=512, n_state=768, n_head=12, n_layer=12, n_ffn=3072, pos_kernel=128, pos_groups=16, num_buckets=320,
                            max_distance=800, stable_layer_norm=0, n_ctx=1500)
WAVLM_LARGE_DIMS = dict(conv_dim=512, n_state=1024, n_head=16, n_layer=24, n_ffn=4096, pos_kernel=128, pos_groups=16, num_buckets=320,
                        max_distance=800, stable_layer_norm=1, n_ctx=1500)
WAVLM_MIN_SAMPLES = 400
# checkpoint tensors that inference never reads (the masking embedding; the heads of the ForCTC / ForXVector / ... wrappers)
WAVLM_IGNORED_PREFIXES = ("masked_spec_embed", "lm_head.", "projector.", "classifier.", "feature_extractor_xvector.", "tdnn.", "objective.",
                          "layer_weights")


def wavlm_dims(name):
    """'base+' (also 'base': the same network) or 'large' -> a copy of the fields of lds_wavlm_cfg"""
    table = {"base": WAVLM_BASE_PLUS_DIMS, "base+": WAVLM_BASE_PLUS_DIMS, "large": WAVLM_LARGE_DIMS}
    if name not in table:
        raise ValueError(f"wavlm_dims: {name!r} (one of {sorted(table)})")
    return dict(table[name])


def wavlm_frames(n_samples):
    """Frames of a clip of n_samples: HuBERT's level rule without padding (400 samples -> 1, 16,000 -> 49, 30 s -> 1499)"""
    return hubert_level_frames(n_samples, 0)[-1]


def wavlm_param_shapes(cfg=None):
    """WavLMModel.state_dict() key -> shape for the tensors inference reads (the names lds_wavlm_create looks up), in the model's order"""
    c = dict(WAVLM_BASE_PLUS_DIMS if cfg is None else cfg)
    D, C, F, K, G, H, NB = c["conv_dim"], c["n_state"], c["n_ffn"], c["pos_kernel"], c["pos_groups"], c["n_head"], c["num_buckets"]
    d = OrderedDict()
    for i in range(7):
        p = f"feature_extractor.conv_layers.{i}."
        d[p + "conv.weight"] = (D, 1 if i == 0 else D, 10 if i == 0 else (3 if i <= 4 else 2))
        if i == 0 or c["stable_layer_norm"]:
            d[p + "layer_norm.weight"] = (D,)
            d[p + "layer_norm.bias"] = (D,)
    d["feature_projection.layer_norm.weight"] = (D,)
    d["feature_projection.layer_norm.bias"] = (D,)
    d["feature_projection.projection.weight"] = (C, D)
    d["feature_projection.projection.bias"] = (C,)
    d["encoder.pos_conv_embed.conv.bias"] = (C,)
    d["encoder.pos_conv_embed.conv.parametrizations.weight.original0"] = (1, 1, K)
    d["encoder.pos_conv_embed.conv.parametrizations.weight.original1"] = (C, C // G, K)
    d["encoder.layer_norm.weight"] = (C,)
    d["encoder.layer_norm.bias"] = (C,)
    for l in range(c["n_layer"]):
        p = f"encoder.layers.{l}."
        d[p + "attention.gru_rel_pos_const"] = (1, H, 1, 1)
        for n in ("k_proj", "v_proj", "q_proj", "out_proj"):
            d[p + f"attention.{n}.weight"] = (C, C)
            d[p + f"attention.{n}.bias"] = (C,)
        d[p + "attention.gru_rel_pos_linear.weight"] = (8, C // H)
        d[p + "attention.gru_rel_pos_linear.bias"] = (8,)
        if l == 0:
            d[p + "attention.rel_attn_embed.weight"] = (NB, H)
        d[p + "layer_norm.weight"] = (C,)
        d[p + "layer_norm.bias"] = (C,)
        d[p + "feed_forward.intermediate_dense.weight"] = (F, C)
        d[p + "feed_forward.intermediate_dense.bias"] = (F,)
        d[p + "feed_forward.output_dense.weight"] = (C, F)
        d[p + "feed_forward.output_dense.bias"] = (C,)
        d[p + "final_layer_norm.weight"] = (C,)
        d[p + "final_layer_norm.bias"] = (C,)
    return d


def wavlm_init_state(cfg=None, seed=0, init_weights=None):
    """Build-owned seeded weights in transformers' names (no checkpoint ships), every stage at a scale of order 1 as in w2v_init_state: the
    feature extractor's convolutions get He's bound sqrt(6 / fan_in), the positional convolution's per-tap norms g lie in [1.5, 3), q_proj and
    k_proj 1.7 times the default bound (attention logits of standard deviation ~3), every norm gain in [0.8, 1.2) and bias in [-0.1, 0.1).
    The relative position bias gets enough weight to matter next to those logits: rel_attn_embed uniform in [-2, 2), gru_rel_pos_linear twice
    the default bound (the two sigmoid arguments have standard deviation ~2.3, so the gate covers most of (1, 2)), gru_rel_pos_const in
    [0.5, 1.5) where the model initialises it to 1; the rest by lds.init_weights' role rules."""
    if init_weights is None:
        from . import init_weights
    import numpy as np
    shapes = wavlm_param_shapes(cfg)
    st = init_weights.init_state(shapes, seed)
    for k, shp in shapes.items():
        fan = int(np.prod(shp[1:])) if len(shp) > 1 else 1
        if "layer_norm." in k:
            st[k] = init_weights.uniform(k, shp, seed, 0.8, 1.2) if k.endswith(".weight") else init_weights.uniform(k, shp, seed, -0.1, 0.1)
        elif k.startswith("feature_extractor.conv_layers.") and k.endswith("conv.weight"):
            b = float(np.sqrt(6.0 / fan))
            st[k] = init_weights.uniform(k, shp, seed, -b, b)
        elif k.endswith("weight.original0"):
            st[k] = init_weights.uniform(k, shp, seed, 1.5, 3.0)
        elif k.endswith("q_proj.weight") or k.endswith("k_proj.weight"):
            b = float(1.7 / np.sqrt(fan))
            st[k] = init_weights.uniform(k, shp, seed, -b, b)
        elif k.endswith("rel_attn_embed.weight"):
            st[k] = init_weights.uniform(k, shp, seed, -2.0, 2.0)
        elif k.endswith("gru_rel_pos_linear.weight"):
            b = float(2.0 / np.sqrt(fan))
            st[k] = init_weights.uniform(k, shp, seed, -b, b)
        elif k.endswith("gru_rel_pos_const"):
            st[k] = init_weights.uniform(k, shp, seed, 0.5, 1.5)
    return OrderedDict((k, np.ascontiguousarray(v, dtype=np.float32)) for k, v in st.items())


XVECTOR_GEOMETRY = dict(tdnn_dim=(512, 512, 512, 512, 1500), tdnn_kernel=(5, 3, 3, 1, 1), tdnn_dilation=(1, 2, 3, 1, 1), xvector_output_dim=512)


def xvector_init_state(D, seed=0, n_layer=None, n_labels=None, geometry=None, init_weights=None):
    """Build-owned seeded weights of an x-vector head (transformers' *ForXVector) over D-wide hidden states, in transformers' names: every
    Linear uniform in +- 1 / sqrt(fan_in) (torch.nn.Linear's default), and with n_layer the raw `layer_weights` of n_layer + 1 hidden states
    uniform in [-1, 1) (non-uniform once soft-maxed).  n_labels: the classifier's outputs, None = xvector_output_dim as in transformers
    (whose config.num_labels sizes the training objective only)."""
    if init_weights is None:
        from . import init_weights
    import numpy as np
    g = dict(XVECTOR_GEOMETRY, **(geometry or {}))
    dims = g["tdnn_dim"]
    st = OrderedDict()

    def lin(name, out, fan_in):
        k = float(1.0 / np.sqrt(fan_in))
        st[f"{name}.weight"] = init_weights.uniform(f"xvector.{name}.weight", (out, fan_in), seed, -k, k)
        st[f"{name}.bias"] = init_weights.uniform(f"xvector.{name}.bias", (out,), seed, -k, k)
    if n_layer is not None:
        st["layer_weights"] = init_weights.uniform("xvector.layer_weights", (n_layer + 1,), seed, -1.0, 1.0)
    lin("projector", dims[0], D)
    for i in range(len(dims)):
        lin(f"tdnn.{i}.kernel", dims[i], (dims[i - 1] if i else dims[0]) * g["tdnn_kernel"][i])
    lin("feature_extractor", g["xvector_output_dim"], 2 * dims[-1])
    lin("classifier", g["xvector_output_dim"] if n_labels is None else n_labels, g["xvector_output_dim"])
    return OrderedDict((k, np.ascontiguousarray(v, dtype=np.float32)) for k, v in st.items())


def wavlm_convert_state(state, cfg=None):
    """A checkpoint's state dict in transformers naming (an optional "module." / "wavlm." prefix removed, masked_spec_embed and the task
    heads dropped) -> the tensors of wavlm_param_shapes(cfg).  A missing tensor is a KeyError naming it; a wrong shape a ValueError."""
    shapes = wavlm_param_shapes(cfg)
    got = {}
    for k, v in state.items():
        for pre in ("module.", "wavlm."):
            if k.startswith(pre):
                k = k[len(pre):]
        if k.startswith(WAVLM_IGNORED_PREFIXES):
            continue
        if k in shapes:
            got[k] = v
    out = OrderedDict()
    for k, shp in shapes.items():
        if k not in got:
            raise KeyError(f"WavLM checkpoint lacks {k!r}")
        if tuple(got[k].shape) != tuple(shp):
            raise ValueError(f"WavLM checkpoint: {k!r} has shape {tuple(got[k].shape)}, expected {tuple(shp)}")
        out[k] = got[k]
    return out


def wavlm_buckets(num_buckets, max_distance, n):
    """WavLMAttention._relative_positions_bucket of the distances -(n - 1) .. n - 1 (key minus query) -> int64 [2 n - 1], the logarithm
    branch in float32 as torch runs it (what lds_wavlm_create builds its bias table from; tests hold the library's table against this)"""
    import numpy as np
    nb, d = num_buckets // 2, np.arange(-(n - 1), n, dtype=np.int64)
    me, a = nb // 2, np.abs(d)
    x = np.log(np.maximum(a, 1).astype(np.float32) / np.float32(me)) / np.float32(np.log(max_distance / me))      # (|d| = 0 takes the small branch)
    big = np.minimum((np.float32(me) + x.astype(np.float32) * np.float32(nb - me)).astype(np.int64), nb - 1)
    return (d > 0) * nb + np.where(a < me, a, big)


RESAMPLE_MAX_RATE, RESAMPLE_MAX_TAPS, RESAMPLE_MAX_BANK = 384000, 1024, 1 << 24      # include/lds.h lds_resample


def resample_bank(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    """The polyphase filter of torchaudio.transforms.Resample(orig_freq, new_freq, "sinc_interp_hann", lowpass_filter_width, rolloff) for
    lds_resample: (O, N, taps, bankT fp32 [taps][N], first int32 [N]).  With O = orig / gcd, N = new / gcd, B = rolloff min(O, N) and the
    integer d = j N - i O (the tap j of phase i sits at d / (O N) periods from the output):
        g(d) = (B / O) sinc(u) cos^2(pi u / (2 w)),   u = clamp(B d / (O N), -w, +w)
    first[i] = the smallest j with |u| < w, taps = the most columns any phase has inside the support, bankT[k][i] = g((first[i] + k) N - i O)
    evaluated in float64 and rounded to fp32 once.  The columns left out sit at the clamp: cos^2(pi / 2) sinc(w), below 1e-30."""
    import math

    import numpy as np
    w = int(lowpass_filter_width)
    if w != lowpass_filter_width or w < 1:
        raise ValueError(f"lowpass_filter_width must be an integer >= 1 (got {lowpass_filter_width})")
    if not 0.0 < rolloff <= 1.0:
        raise ValueError(f"rolloff must be in (0, 1] (got {rolloff})")
    for f in (orig_freq, new_freq):
        if int(f) != f or not 1 <= f <= RESAMPLE_MAX_RATE:
            raise ValueError(f"sample rates must be integers in 1 .. {RESAMPLE_MAX_RATE} (got {orig_freq}, {new_freq})")
    g = math.gcd(int(orig_freq), int(new_freq))
    O, N = int(orig_freq) // g, int(new_freq) // g
    base = min(O, N) * float(rolloff)
    half = w * O * N / base                                     # the support is |d| < half
    i = np.arange(N, dtype=np.int64)
    j0 = np.floor((i * O - half) / N).astype(np.int64) + 1      # smallest j with j N - i O > -half, made exact against float rounding:
    j0 += (j0 * N - i * O) <= -half
    j0 -= ((j0 - 1) * N - i * O) > -half
    j1 = np.ceil((i * O + half) / N).astype(np.int64) - 1       # largest j with j N - i O < half
    j1 -= (j1 * N - i * O) >= half
    j1 += ((j1 + 1) * N - i * O) < half
    taps = int((j1 - j0 + 1).max())
    if taps > RESAMPLE_MAX_TAPS or N * taps > RESAMPLE_MAX_BANK:
        raise ValueError(f"resampling {orig_freq} -> {new_freq} needs {taps} taps x {N} phases; at most {RESAMPLE_MAX_TAPS} taps and "
                         f"{RESAMPLE_MAX_BANK} bank entries are built")
    d = (j0[None, :] + np.arange(taps, dtype=np.int64)[:, None]) * N - (i * O)[None, :]      # [taps][N]
    u = np.clip(base * d / (O * N), -float(w), float(w))
    bank = (base / O) * np.sinc(u) * np.cos(np.pi * u / (2.0 * w)) ** 2
    return O, N, taps, np.ascontiguousarray(bank, dtype=np.float32), np.ascontiguousarray(j0, dtype=np.int32)
