"""The ragged VAE encoder (Hifi_VAEGAN.extract_ragged, include/lds.h lds_vae_encoder_forward_ragged) on the GPU: every clip of a padded
batch against the same clip encoded alone, zeros beyond each clip's frames, the plain path's bits when nothing is ragged, whatever the
buffer, the noise or the workspace hold beyond the clips, and the strided convolution's masks (csrc/conv_down.hip) against numpy under
every tile."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HOP = 512
H_RB2 = dict(resblock="2", resblock_dilation_sizes=[[1, 3], [1, 3], [1, 3]])
# one buffer of 40 frames: the full buffer, one sample, one sample past a hop (T_b = 38), a length no stage's stride divides, 513
LENS = [40 * HOP, 1, 37 * HOP + 1, HOP + 1, 23 * HOP - 7]
TOL = 1e-5


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def relmax(got, ref):
    return float(np.abs(got.astype(np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


def frames(n):
    return -(-n // HOP)


def _h(rb):
    from lds import arch
    return arch.SYNTHETIC_VOCODER_H if rb == "1" else dict(arch.SYNTHETIC_VOCODER_H, **H_RB2)


def _vae(h, seed=0):
    from encoder.hifi_vaegan.hifi_vaegan import Hifi_VAEGAN
    from lds import arch, init_weights
    return Hifi_VAEGAN(None, device="cuda", h=h, state={}, encoder_state=init_weights.init_state(arch.encoder_param_shapes(h), seed))


def _audio(tag, lens, L, fill):
    """[B, L] with the clips' samples from the seeded generator and `fill` beyond each length (garbage the encoder must never see)"""
    from lds import init_weights
    a = init_weights.uniform(tag, (len(lens), L), 71, -0.5, 0.5)
    for b, n in enumerate(lens):
        if isinstance(fill, str):      # "garbage": large values with NaN and Inf among them
            g = init_weights.uniform(tag + ".g", (L - n,), 72, -1e6, 1e6)
            g[::7] = np.nan
            g[3::11] = np.inf
            a[b, n:] = g
        else:
            a[b, n:] = fill
    return a


def _alone(vae, audio, n, **kw):
    """clip audio[b, :n] through the plain extract, on its own"""
    return vae.extract(audio[None, :n].contiguous(), **kw)[0].cpu().numpy()


@pytest.mark.parametrize("rb", ["1", "2"])
def test_ragged_vs_alone(rb, record_margin):
    """B = 5 clips in one 40-frame buffer with garbage beyond them: every clip's rows match the clip encoded alone, the rows beyond are
    exact zeros, nothing is non-finite"""
    vae = _vae(_h(rb))
    audio = dev(_audio("rg.enc.audio", LENS, 40 * HOP, "garbage"))
    out = vae.extract_ragged(audio, LENS, noise=torch.zeros(5, 80, 40, device="cuda"))
    assert out.shape == (5, 40, 160)
    assert torch.isfinite(out).all()
    out = out.cpu().numpy()
    worst = 0.0
    for b, n in enumerate(LENS):
        T = frames(n)
        ref = _alone(vae, audio[b], n, noise=torch.zeros(1, 80, T, device="cuda"))
        assert ref.shape == (T, 160)
        worst = max(worst, relmax(out[b, :T], ref))
        assert not out[b, T:].any(), b
    record_margin(worst, TOL)


@pytest.mark.parametrize("mode", ["default", "only_mean", "only_z"])
def test_ragged_all_full_lengths_is_the_plain_path_bit_for_bit(mode):
    from lds import init_weights
    vae = _vae(_h("1"))
    L = 37 * HOP
    audio = dev(init_weights.uniform("full.enc.audio", (3, L), 73, -0.5, 0.5))
    noise = dev(init_weights.uniform("full.enc.noise", (3, 80, 37), 74, -2.0, 2.0))
    kw = dict(only_mean=mode == "only_mean", only_z=mode == "only_z", noise=noise)
    plain = vae.extract(audio, **kw)
    got = vae.extract_ragged(audio, [L] * 3, **kw)
    assert torch.equal(got, plain)


@pytest.mark.parametrize("rb", ["1", "2"])
def test_ragged_only_z_uses_each_clips_own_noise(rb, record_margin):
    """z[b, :T_b] = the clip's z alone with noise[b, :, :T_b]; the noise beyond T_b (NaN here) is never read, z beyond T_b is zero"""
    from lds import init_weights
    vae = _vae(_h(rb))
    audio = dev(_audio("rgz.enc.audio", LENS, 40 * HOP, "garbage"))
    noise = init_weights.uniform("rgz.enc.noise", (5, 80, 40), 75, -2.0, 2.0)
    for b, n in enumerate(LENS):
        noise[b, :, frames(n):] = np.nan
    noise = dev(noise)
    z = vae.extract_ragged(audio, LENS, only_z=True, noise=noise)
    assert z.shape == (5, 40, 80) and torch.isfinite(z).all()
    z = z.cpu().numpy()
    worst = 0.0
    for b, n in enumerate(LENS):
        T = frames(n)
        ref = _alone(vae, audio[b], n, only_z=True, noise=noise[b:b + 1, :, :T].contiguous())
        worst = max(worst, relmax(z[b, :T], ref))
        assert not z[b, T:].any(), b
    record_margin(worst, TOL)


def test_ragged_padding_contents_are_irrelevant():
    """the same clips with zeros, NaN or +1e30 beyond their lengths give the same bits"""
    vae = _vae(_h("1"))
    noise = torch.zeros(5, 80, 40, device="cuda")
    outs = [vae.extract_ragged(dev(_audio("pad.enc.audio", LENS, 40 * HOP, f)), LENS, noise=noise) for f in (0.0, np.nan, 1e30)]
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[1], outs[0]) and torch.equal(outs[2], outs[0])


@pytest.mark.parametrize("pattern", [0x7FC00000, 0x7F800000, 0xFF800000])
def test_ragged_poisoned_workspace(pattern):
    """a workspace full of NaN / +Inf / -Inf gives the bits of a clean one on the ragged path"""
    from lds import init_weights, native
    vae = _vae(_h("1"))
    audio = dev(_audio("rpoison.enc.audio", LENS, 40 * HOP, "garbage"))
    noise = dev(init_weights.uniform("rpoison.enc.noise", (5, 80, 40), 76, -2.0, 2.0))
    clean_out = vae.extract_ragged(audio, LENS, noise=noise)
    clean_z = vae.extract_ragged(audio, LENS, only_z=True, noise=noise)
    enc = vae.encoder_model
    ws = torch.empty(enc.workspace_bytes(5, 40 * HOP), dtype=torch.uint8, device="cuda")
    native.debug_fill(ws, pattern)
    out, z = enc.forward(audio, noise, ws=ws, lengths=LENS)
    assert torch.equal(out, clean_out) and torch.equal(z, clean_z)


# ---- the strided convolution's masks alone ---------------------------------------------------------------------------------------
SHAPES = [      # (Ci, Co, K, stride, slope): conv_pre, the five downsamplers of the config, conv_post
    (1, 16, 7, 1, 1.0), (16, 32, 4, 2, 0.1), (32, 64, 4, 2, 0.1), (64, 128, 4, 2, 0.1), (128, 256, 16, 8, 0.1), (256, 512, 16, 8, 0.1),
    (512, 160, 7, 1, 0.01)]


@pytest.mark.parametrize("Ci,Co,K,stride,slope", SHAPES)
def test_conv_down_ragged_vs_numpy_every_tile(Ci, Co, K, stride, slope, record_margin):
    """4 elements x 300 output frames (three to five column tiles): full lengths; one frame; lengths that end inside a tile; no output at all.
    NaN beyond every input length.  Every forced tile gives the same bits; they are the plain kernel's bits on the zeroed input up to
    lengths_out, zeros beyond, and match numpy."""
    from lds import init_weights, native
    from oracle import vocoder as o_voc
    from oracle.unet1d import conv1d
    B, To = 4, 300
    T = To * stride
    lin = [T, 3, 131 * stride - 1, 7 * stride]
    lout = [To, 1, 130, 0]
    x = init_weights.uniform(f"cdr.x.{Ci}.{K}", (B, Ci, T), 80, -1.0, 1.0)
    x0 = x.copy()
    for b, n in enumerate(lin):
        x[b, :, n:] = np.nan
        x0[b, :, n:] = 0.0
    w = init_weights.uniform(f"cdr.w.{Ci}.{K}", (Co, Ci, K), 81, -1.0, 1.0) / np.float32(np.sqrt(Ci * K))
    bias = init_weights.uniform(f"cdr.b.{Ci}.{K}", (Co,), 82, -0.1, 0.1)
    xd = dev(x)
    outs = {}
    for tile in (64064, 64128, 128128, 0):
        cfg = []
        outs[tile] = native.conv_down_ragged(xd, w, bias, stride, lin, lout, slope, tile=tile, cfg=cfg).cpu().numpy()
        if tile:
            assert cfg[0].startswith(f"BM{tile // 1000} BN{tile % 1000} "), cfg
    for tile in (64128, 128128, 0):
        assert np.array_equal(outs[tile], outs[64064]), tile
    got = outs[0]
    plain = native.conv_down(dev(x0), w, bias, stride, slope).cpu().numpy()
    ref = conv1d(o_voc.lrelu(x0, slope).astype(np.float64), w.astype(np.float64), bias.astype(np.float64), stride=stride, pad=(K - stride + 1) // 2)
    assert got.shape == plain.shape == ref.shape == (B, Co, To)
    for b, n in enumerate(lout):
        assert np.array_equal(got[b, :, :n], plain[b, :, :n]), b
        assert not got[b, :, n:].any(), b
        ref[b, :, n:] = 0.0
    record_margin(relmax(got, ref), TOL)


# ---- the bench's shape -----------------------------------------------------------------------------------------------------------
def test_ragged_bench_size_row(record_margin):
    """16 clips of 16 lengths (272 .. 512 frames, none a multiple of the hop) in one 512-frame buffer: every stage ragged at B = 16,
    the 512-channel stage included; the shortest and the longest clip against their stand-alone runs"""
    from lds import init_weights
    vae = _vae(_h("1"))
    lens = [(272 + 16 * i) * HOP - 37 for i in range(16)]
    audio = dev(init_weights.uniform("rbench.enc.audio", (16, 512 * HOP), 77, -0.5, 0.5))
    out = vae.extract_ragged(audio, lens, noise=torch.zeros(16, 80, 512, device="cuda"))
    assert torch.isfinite(out).all()
    out = out.cpu().numpy()
    worst = 0.0
    for b in (0, 15):
        T = frames(lens[b])
        ref = _alone(vae, audio[b], lens[b], noise=torch.zeros(1, 80, T, device="cuda"))
        worst = max(worst, relmax(out[b, :T], ref))
    for b, n in enumerate(lens):
        assert not out[b, frames(n):].any(), b
    record_margin(worst, TOL)
