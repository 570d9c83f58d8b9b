"""The diffusion loss of the validation pass on the GPU (GaussianDiffusion.p_losses / forward(infer=False); include/lds.h lds_q_sample_rows,
lds_loss_reduce) against what the reference's p_losses made of the same inputs (tests/golden/diffusion_loss.npz), and tools/validate.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def model():
    from diffusion.unit2mel import Unit2Mel
    return Unit2Mel(1280, 323, 80).to("cuda").eval()


@pytest.fixture(scope="module")
def fx(golden):
    return golden("diffusion_loss.npz")


def _loss(gd, g, loss_type):
    return gd.p_losses(dev(g["x_start"]), dev(g["t"]), dev(g["cond"]), noise=dev(g["noise"]), loss_type=loss_type)


@pytest.mark.parametrize("loss_type", ["l2", "l1"])
def test_p_losses_vs_reference(model, fx, loss_type):
    from lds import native
    gd, g = model.decoder, fx
    loss = _loss(gd, g, loss_type)
    assert loss.dim() == 0 and loss.is_cuda and loss.dtype == torch.float32
    # the three stages p_losses is made of, run by hand: their result is the loss, bit for bit
    x0, nz = dev(g["x_start"][:, 0]), dev(g["noise"][:, 0])
    x_noisy, tf = native.q_sample_rows(x0, nz, dev(g["t"]), gd.sqrt_alphas_cumprod, gd.sqrt_one_minus_alphas_cumprod)
    # q_sample: the reference's bits (t = 0, 517, 999 gathered on the device, two roundings and a sum)
    assert torch.equal(x_noisy.cpu(), torch.from_numpy(g["x_noisy"])) and torch.equal(tf.cpu(), torch.from_numpy(g["t"].astype(np.float32)))
    # the denoiser inside p_losses is lds_unet_forward on (x_noisy, t as fp32)
    eps = gd.denoise_fn.native().forward(x_noisy, dev(g["cond"]), tf)
    assert torch.equal(native.loss_reduce(nz, eps, loss_type), loss)
    # the reduction against a float64 mean of the native residual
    noise = g["noise"].reshape(eps.shape)
    res = noise.astype(np.float32) - eps.cpu().numpy()
    mean64 = float((res.astype(np.float64) ** 2).mean() if loss_type == "l2" else np.abs(res.astype(np.float64)).mean())
    got = float(loss)
    print(f"{loss_type}: loss {got!r}, mean64 {mean64!r}, reference {float(g['loss_' + loss_type])!r}")
    assert abs(got - mean64) <= 1e-6 * got
    # against the reference: first order in the UNet's tolerance 2e-5 * absmax (d mean(r^2) = 2 mean(|r| d), d mean(|r|) <= d)
    ref, d = float(g["loss_" + loss_type]), 2e-5 * float(np.abs(g["eps_ref"]).max())
    bound = (2 * d * float(np.abs(noise - g["eps_ref"]).mean()) if loss_type == "l2" else d) + 1e-6 * ref
    print(f"{loss_type}: |loss - ref| {abs(got - ref):.3e}, bound {bound:.3e}")
    assert abs(got - ref) <= bound
    for _ in range(2):
        assert torch.equal(_loss(gd, g, loss_type), loss)
    assert torch.equal(native.loss_reduce(dev(noise), eps, loss_type, ws=torch.full((4096,), 0xFF, dtype=torch.uint8, device="cuda")), loss)


def test_loss_reduce_sizes():
    """one element, a slice and one more, several slices with a ragged end: the double mean of the fp32 residual"""
    from lds import native
    rng = np.random.RandomState(5)
    for n in (1, 4096, 4097, 3 * 4096 + 77):
        a, b = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
        r = (a - b).astype(np.float64)
        for lt, ref in (("l2", ((a - b) * (a - b)).astype(np.float64).mean()), ("l1", np.abs(r).mean())):
            got = float(native.loss_reduce(dev(a), dev(b), lt))
            assert abs(got - ref) <= 2.0 ** -23 * ref, (n, lt, got, ref)


def test_forward_infer_false(model, fx):
    g = fx
    units = dev(np.random.RandomState(1).uniform(-1.7, 1.7, size=(3, 40, 1280)).astype(np.float32))
    spk = torch.tensor([[7], [1], [323]], device="cuda")
    gt = dev(g["x_start"][:, 0].transpose(0, 2, 1))      # [B,T,M]
    torch.manual_seed(11)
    a = model(units, None, spk_id=spk, gt_spec=gt, infer=False)
    assert a.dim() == 0 and bool(torch.isfinite(a)) and float(a) > 0
    torch.manual_seed(11)
    assert torch.equal(model(units, None, spk_id=spk, gt_spec=gt, infer=False), a)
    # both draws injected: the loss of the decoder's p_losses on the embedded condition, and no draw is consumed
    t, noise = dev(g["t"]), dev(g["noise"])
    state = torch.cuda.get_rng_state()
    b = model.loss(units, None, spk_id=spk, gt_spec=gt, t=t, noise=noise)
    assert torch.equal(torch.cuda.get_rng_state(), state)
    assert torch.equal(model.loss(units, None, spk_id=spk, gt_spec=gt, t=t, noise=noise), b)
    with pytest.raises(NotImplementedError):
        model.loss(units, None, spk_id=spk, gt_spec=gt, t=t, noise=noise, loss_type="huber")
    with pytest.raises(NotImplementedError):
        model.decoder.p_losses(dev(g["x_start"]), t, dev(g["cond"]), loss_type="huber")


def test_validate_tool_synthetic(tmp_path):
    out = tmp_path / "val.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "validate.py"), "--synthetic", "--items", "2", "--frames", "24", "--method", "unipc",
                        "--speedup", "250", "--out", str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    res = json.load(open(out))
    assert len(res["items"]) == 2 and all(np.isfinite(it["loss"]) and np.isfinite(it["mel_l1"]) and it["frames"] == 24 for it in res["items"])
    assert np.isfinite(res["loss"]) and np.isfinite(res["mel_l1"])
    assert abs(res["loss"] - np.mean([it["loss"] for it in res["items"]])) < 1e-6
