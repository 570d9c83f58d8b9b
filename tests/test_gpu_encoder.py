"""The HiFi-VAEGAN encoder (audio -> latent; include/lds.h lds_vae_encoder_*, csrc/conv_down.hip) on the GPU: parity with the reference's
own Hifi_VAEGAN.extract (tests/golden/encoder*.npz), with a numpy restatement at full size and in partial tiles, the strided
convolution alone at every shape of the config, poisoned workspaces, repeatability, and the decoder's output unchanged by the MRF
refactor that the encoder shares."""
import functools
import hashlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def relmax(got, ref):
    return float(np.abs(got.astype(np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


def _vae(h, seed=0):
    from encoder.hifi_vaegan.hifi_vaegan import Hifi_VAEGAN
    from lds import arch, init_weights
    return Hifi_VAEGAN(None, device="cuda", h=h, state={}, encoder_state=init_weights.init_state(arch.encoder_param_shapes(h), seed))


# ---- numpy restatement of reference models.py:39-54 (oracle/ building blocks only) ------------------------------------------------
def encoder_forward_np(w_folded, h, audio):
    """audio [B, L] (L a multiple of the hop) -> (m, logs) [B, C, T]"""
    from oracle import vocoder as o_voc
    from oracle.unet1d import conv1d
    w = w_folded
    f32 = np.float32
    x = conv1d(audio[:, None, :].astype(f32), w["conv_pre.weight"], w["conv_pre.bias"], pad=3)
    nk = len(h["resblock_kernel_sizes"])
    rb = o_voc.resblock1 if h["resblock"] == "1" else o_voc.resblock2
    for i, (u, k) in enumerate(zip(reversed(h["upsample_rates"]), reversed(h["upsample_kernel_sizes"]))):
        x = conv1d(o_voc.lrelu(x), w[f"ups.{i}.weight"], w[f"ups.{i}.bias"], stride=u, pad=(k - u + 1) // 2)
        xs = None
        for j, (kk, dil) in enumerate(zip(h["resblock_kernel_sizes"], h["resblock_dilation_sizes"])):
            y = rb(w, f"resblocks.{i * nk + j}.", x, kk, dil)
            xs = y if xs is None else (xs + y).astype(f32)
        x = (xs / f32(nk)).astype(f32)
    x = conv1d(o_voc.lrelu(x, 0.01), w["conv_post.weight"], w["conv_post.bias"], pad=3)
    C = h["inter_channels"]
    return x[:, :C], x[:, C:]


# ---- reference parity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixture", ["encoder.npz", "encoder_rb2.npz"])
@pytest.mark.parametrize("mode", ["default", "only_mean", "only_z"])
def test_encoder_vs_reference(golden, record_margin, fixture, mode):
    import json
    g = golden(fixture)
    h = json.loads(bytes(g["h_json"]).decode())
    vae = _vae(h)
    audio = dev(g["audio"])
    if mode == "default":
        got, ref = vae.extract(audio, noise=dev(g["noise"])), g["out"]
    elif mode == "only_mean":
        got, ref = vae.extract(audio, only_mean=True, noise=dev(g["noise_mean"])), g["out_mean"]
    else:
        got, ref = vae.extract(audio, only_z=True, only_mean=True, noise=dev(g["noise_z"])), g["z_mean"]
    got = got.cpu().numpy()
    assert got.shape == ref.shape
    if mode == "only_mean":
        assert not got[..., h["inter_channels"]:].any()
    record_margin(relmax(got, ref), 1e-4)


def test_vocoder_extract_draws_like_the_reference():
    """Vocoder.extract -> Hifi_VAEGAN.extract; every call draws randn of m's shape [B, C, T] on the device (randn_like(m)), so the
    torch generator advances exactly as in the reference; only_z uses that draw"""
    from diffusion.vocoder import Vocoder
    from lds import arch, init_weights
    h = arch.SYNTHETIC_VOCODER_H
    voc = Vocoder.__new__(Vocoder)
    voc.vocoder = _vae(h)
    voc.vocoder_sample_rate, voc.vocoder_hop_size, voc.dimension = 44100, 512, 80
    audio = dev(init_weights.uniform("enc.api.audio", (2, 5 * 512 - 7), 3, -0.5, 0.5))
    torch.manual_seed(123)
    z = voc.extract(audio, 44100, only_z=True)
    after = torch.randn(4, device="cuda")
    torch.manual_seed(123)
    n = torch.randn(2, 80, 5, device="cuda")
    assert torch.equal(torch.randn(4, device="cuda"), after)
    assert torch.equal(z, voc.vocoder.extract(audio, only_z=True, noise=n))
    torch.manual_seed(5)
    out = voc.extract(audio, 44100)      # the default mode draws too (the reference computes z in every call)
    assert out.shape == (2, 5, 160)
    after2 = torch.randn(4, device="cuda")
    torch.manual_seed(5)
    torch.randn(2, 80, 5, device="cuda")
    assert torch.equal(torch.randn(4, device="cuda"), after2)
    with pytest.raises(ValueError, match="keyshift"):
        voc.extract(audio, 44100, keyshift=2)
    with pytest.raises(ValueError, match="22050.*44100"):
        voc.extract(audio, 22050)


# ---- full size and partial tiles vs the numpy restatement ----------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _full512():
    """one utterance of 512 frames (262,144 samples) and its restatement [1, 512, 2C] (~20 s of CPU, shared by two tests)"""
    from lds import arch, init_weights
    from oracle import vocoder as o_voc
    h = arch.SYNTHETIC_VOCODER_H
    state = init_weights.init_state(arch.encoder_param_shapes(h), 0)
    audio = init_weights.uniform("full512.enc.audio", (1, 512 * 512), 45, -0.5, 0.5)
    m, logs = encoder_forward_np(o_voc.fold_weight_norm(state), h, audio)
    return audio, np.concatenate([m, logs], axis=1).transpose(0, 2, 1)


def test_encoder_512_frames_vs_numpy(record_margin):
    """one utterance of 512 frames (262,144 samples), alone: every stage at B = 1's tile shapes (32@131072 ... 512@512 columns)"""
    from lds import arch
    vae = _vae(arch.SYNTHETIC_VOCODER_H)
    audio, ref = _full512()
    got = vae.extract(dev(audio), noise=torch.zeros(1, 80, 512, device="cuda")).cpu().numpy()
    assert got.shape == ref.shape == (1, 512, 160)
    record_margin(relmax(got, ref), 1e-4)


@pytest.mark.parametrize("rb", ["1", "2"])
def test_encoder_partial_tiles_vs_numpy_and_alone(rb, record_margin):
    """2 x 37 frames: every stage ends in a partial tile; z against the restatement with the same noise; each utterance encoded alone
    gives the bits it gets inside the batch"""
    from lds import arch, init_weights
    from oracle import vocoder as o_voc
    h = arch.SYNTHETIC_VOCODER_H if rb == "1" else dict(arch.SYNTHETIC_VOCODER_H, resblock="2", resblock_dilation_sizes=[[1, 3], [1, 3], [1, 3]])
    state = init_weights.init_state(arch.encoder_param_shapes(h), 0)
    vae = _vae(h)
    audio = init_weights.uniform("p37.enc.audio", (2, 37 * 512), 46, -0.5, 0.5)
    noise = init_weights.uniform("p37.enc.noise", (2, 80, 37), 47, -2.0, 2.0)
    z = vae.extract(dev(audio), only_z=True, noise=dev(noise)).cpu().numpy()
    out = vae.extract(dev(audio), noise=dev(noise)).cpu().numpy()
    m, logs = encoder_forward_np(o_voc.fold_weight_norm(state), h, audio)
    ref = np.concatenate([m, logs], axis=1).transpose(0, 2, 1)
    zref = (m.astype(np.float64) + noise * np.exp(logs.astype(np.float64))).transpose(0, 2, 1)
    record_margin(relmax(out, ref), 1e-4, "out")
    record_margin(relmax(z, zref), 1e-4, "z")
    for b in range(2):
        alone = vae.extract(dev(audio[b:b + 1]), noise=dev(noise[b:b + 1])).cpu().numpy()
        assert np.array_equal(alone[0], out[b])


# ---- the strided convolution alone ---------------------------------------------------------------------------------------------
SHAPES = [      # (Ci, Co, K, stride, slope): conv_pre, the five downsamplers of the config, conv_post
    (1, 16, 7, 1, 1.0), (16, 32, 4, 2, 0.1), (32, 64, 4, 2, 0.1), (64, 128, 4, 2, 0.1), (128, 256, 16, 8, 0.1), (256, 512, 16, 8, 0.1),
    (512, 160, 7, 1, 0.01)]


@pytest.mark.parametrize("Ci,Co,K,stride,slope", SHAPES)
@pytest.mark.parametrize("B,Tout", [(3, 37), (1, 300)])
def test_conv_down_vs_numpy(Ci, Co, K, stride, slope, B, Tout, record_margin):
    from lds import init_weights, native
    from oracle import vocoder as o_voc
    from oracle.unet1d import conv1d
    T = Tout * stride
    x = init_weights.uniform(f"cd.x.{Ci}.{K}", (B, Ci, T), 50, -1.0, 1.0)
    w = init_weights.uniform(f"cd.w.{Ci}.{K}", (Co, Ci, K), 51, -1.0, 1.0) / np.float32(np.sqrt(Ci * K))
    b = init_weights.uniform(f"cd.b.{Ci}.{K}", (Co,), 52, -0.1, 0.1)
    got = native.conv_down(dev(x), w, b, stride, slope).cpu().numpy()
    xa = o_voc.lrelu(x, slope).astype(np.float64)
    ref = conv1d(xa, w.astype(np.float64), b.astype(np.float64), stride=stride, pad=(K - stride + 1) // 2)
    assert got.shape == ref.shape == (B, Co, Tout)
    record_margin(relmax(got, ref), 1e-5)      # fp32 accumulation over Ci * K <= 4096 products: 2-3e-6 at the longest reductions


def _tile_rule(Co, To, B):
    """kernels' own rule (csrc/conv_down.hip launch_conv_down), judged against this device's CU count"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    blocks = lambda bm, bn: -(-Co // bm) * -(-To // bn) * B      # noqa: E731
    if Co > 64 and blocks(128, 128) >= 2 * cus:
        return "BM128 BN128"
    return "BM64 BN128" if blocks(64, 128) >= cus else "BM64 BN64"


@pytest.mark.parametrize("Ci,Co,K,stride,B,Tout", [(64, 128, 4, 2, 2, 32768), (128, 256, 16, 8, 2, 16384), (256, 512, 16, 8, 3, 37)])
def test_conv_down_every_tile_vs_numpy(Ci, Co, K, stride, B, Tout, record_margin):
    """every tile configuration (64x64, 64x128, 128x128) forced on the same data gives the same bits, and those bits match numpy; at the
    first two shapes (ups.2 / ups.3 with >= 512 workgroups of 128 x 128) the product path's own choice is the 128 x 128 tile on a 256-CU
    device"""
    from lds import init_weights, native
    from oracle import vocoder as o_voc
    from oracle.unet1d import conv1d
    T = Tout * stride
    x = init_weights.uniform(f"cdt.x.{Ci}.{K}", (B, Ci, T), 60, -1.0, 1.0)
    w = init_weights.uniform(f"cdt.w.{Ci}.{K}", (Co, Ci, K), 61, -1.0, 1.0) / np.float32(np.sqrt(Ci * K))
    b = init_weights.uniform(f"cdt.b.{Ci}.{K}", (Co,), 62, -0.1, 0.1)
    xd = dev(x)
    outs = {}
    for tile in (64064, 64128, 128128, 0):
        cfg = []
        outs[tile] = native.conv_down(xd, w, b, stride, 0.1, tile=tile, cfg=cfg).cpu().numpy()
        if tile:
            assert cfg[0].startswith(f"BM{tile // 1000} BN{tile % 1000} "), cfg
        else:
            assert cfg[0].startswith(_tile_rule(Co, Tout, B) + " "), cfg
    for tile in (64128, 128128, 0):
        assert np.array_equal(outs[tile], outs[64064]), tile
    if Tout > 1000 and torch.cuda.get_device_properties(0).multi_processor_count == 256:
        assert _tile_rule(Co, Tout, B) == "BM128 BN128"
    ref = conv1d(o_voc.lrelu(x, 0.1).astype(np.float64), w.astype(np.float64), b.astype(np.float64), stride=stride, pad=(K - stride + 1) // 2)
    assert outs[0].shape == ref.shape == (B, Co, Tout)
    record_margin(relmax(outs[128128], ref), 1e-5)


# ---- workspace poisoning, repeatability ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", [0x7FC00000, 0x7F800000, 0xFF800000])
def test_encoder_poisoned_workspace(pattern):
    """a workspace full of NaN / +Inf / -Inf gives the bits of a clean one: nothing reads what the call did not write"""
    from lds import init_weights, native, arch
    h = arch.SYNTHETIC_VOCODER_H
    vae = _vae(h)
    audio = dev(init_weights.uniform("poison.enc.audio", (3, 37 * 512), 48, -0.5, 0.5))
    noise = dev(init_weights.uniform("poison.enc.noise", (3, 80, 37), 49, -2.0, 2.0))
    clean_out, clean_z = vae.extract(audio, noise=noise), vae.extract(audio, only_z=True, noise=noise)
    enc = vae.encoder_model
    ws = torch.empty(enc.workspace_bytes(3, 37 * 512), dtype=torch.uint8, device="cuda")
    native.debug_fill(ws, pattern)
    out, z = enc.forward(audio, noise, ws=ws)
    assert torch.equal(out, clean_out) and torch.equal(z, clean_z)


def test_encoder_batch16_vs_numpy_and_repeatable(record_margin):
    """the bench's shape, 16 x 512 frames, where the tile rules pick the batch's tiles (conv_down 128 x 128 for ups.2 / ups.3): row 0 is
    the 512-frame utterance of test_encoder_512_frames_vs_numpy, checked against the restatement; five encodes are bit-identical"""
    from lds import arch, init_weights
    h = arch.SYNTHETIC_VOCODER_H
    vae = _vae(h)
    a0, ref = _full512()
    audio = init_weights.uniform("rep.enc.audio", (16, 512 * 512), 53, -0.5, 0.5)
    audio[0] = a0[0]
    audio = dev(audio)
    noise = torch.zeros(16, 80, 512, device="cuda")
    first = vae.extract(audio, noise=noise)
    assert torch.isfinite(first).all()
    record_margin(relmax(first[:1].cpu().numpy(), ref), 1e-4)
    for _ in range(4):
        assert torch.equal(vae.extract(audio, noise=noise), first)


# ---- the decoder is unchanged by the shared MRF code --------------------------------------------------------------------------
DECODER_SHA256 = "58642d0f5d7ea2f6fa2d7a64877f6db559b63e021c543bd3aa336dd4fe4e799f"      # the library of the parent commit


def test_decoder_output_unchanged_by_the_encoder():
    """16 x 512 frames through the decoder, hashed: the value was taken with the library before the encoder shared its stage code"""
    from encoder.hifi_vaegan.hifi_vaegan import Hifi_VAEGAN
    from lds import arch, init_weights
    h = arch.SYNTHETIC_VOCODER_H
    voc = Hifi_VAEGAN(None, device="cuda", h=h, state=init_weights.init_state(arch.generator_param_shapes(h), 0))
    z = init_weights.uniform("hash.voc.z", (16, 512, 80), 7, -1.5, 1.5)
    wav = voc(dev(z)).cpu().numpy()
    assert wav.shape == (16, 1, 262144)
    assert hashlib.sha256(wav.tobytes()).hexdigest() == DECODER_SHA256
