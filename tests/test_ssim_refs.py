"""CPU: the plain-torch restatement of the SSIM criterion (tests/ssim_refs.py) is the validation metric, is exact on identical
constant images, differentiates correctly, and its anti-correlated case really has N2 < 0.  Also: the three-map form of the gradient
that csrc/ssim_loss.hip computes equals autograd of the restatement."""
import numpy as np
import pytest
import torch

import ssim_refs as sr_
from conftest import rel_err


def _host_ssim(sr, hr):
    """SSIM of validate.image_metrics: utils.SSIM on the Y channel of the uint8 images, 0..255 scale."""
    from srganst.utils import SSIM, bgr2ycbcr, tensor2img
    a = bgr2ycbcr(tensor2img(sr).astype(np.float32) / 255.0, only_y=True)
    b = bgr2ycbcr(tensor2img(hr).astype(np.float32) / 255.0, only_y=True)
    return SSIM(a * 255, b * 255)


@pytest.mark.parametrize("seed, H, W", [(9, 60, 52), (10, 11, 37)])
def test_restatement_is_the_validation_metric_on_grid_images(seed, H, W):
    """SSIM is scale-consistent (C1, C2 scale with the square of the range), so on clamped 1/255-grid images 1 - loss("y") in fp64 is
    what validate reports; 1e-7 absorbs the host path's fp32 rounding of Y (measured 2e-9)."""
    x, gt = (sr_.on_grid(t) for t in sr_.images(seed, 1, H, W))
    host = _host_ssim(x[0], gt[0])
    ref = 1.0 - sr_.ssim_loss(x.double(), gt.double(), "y").item()
    print(f"[{H}x{W}] host SSIM {host:.12f} restatement {ref:.12f} diff {abs(host - ref):.2e}")
    assert host < 0.999                                  # sr and gt differ: the agreement is not that of 1 with 1
    assert abs(host - ref) <= 1e-7


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("channel", ["y", "rgb"])
def test_identical_constant_images_have_zero_loss(channel, dtype):
    z = torch.full((2, 3, 17, 23), 0.3, dtype=dtype)
    z[:, 1] = 0.7
    assert sr_.ssim_loss(z, z.clone(), channel).item() == 0.0


@pytest.mark.parametrize("channel", ["y", "rgb"])
def test_gradcheck_fp64(channel):
    x, gt = sr_.images(3, 1, 12, 13)
    xd = x.double().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: sr_.ssim_loss(t, gt.double(), channel), (xd,), eps=1e-6, atol=1e-7, rtol=1e-5)


@pytest.mark.parametrize("channel", ["y", "rgb"])
def test_anti_correlated_case_has_negative_n2(channel):
    x, gt, *_ = sr_.case("anti-correlated", channel)
    frac = sr_.n2_negative_fraction(x, gt, channel)
    print(f"[{channel}] N2 < 0 at {frac:.2%} of the positions")
    assert frac >= 0.01
    for name in sr_.CASES:
        if name != "anti-correlated":
            x2, gt2, *_ = sr_.case(name, channel)
            assert sr_.n2_negative_fraction(x2, gt2, channel) < frac


@pytest.mark.parametrize("channel", ["y", "rgb"])
@pytest.mark.parametrize("name", list(sr_.CASES))
def test_three_map_gradient_equals_autograd(name, channel):
    """The backward the kernels implement - three maps, formed without a division by N1 or N2, filtered by a full correlation and
    combined with x[q], y[q] - against autograd, both in fp64; and the fp32 restatement stays within 1e-4 of fp64 on every case, so
    the 1e-3 floor of the fp64-truth rule is the binding bound of the GPU tests."""
    x, gt, l32, g32, l64, g64 = sr_.case(name, channel)
    g = sr_.grad_from_maps(x.double(), gt.double(), channel)
    e = rel_err(g, g64)
    print(f"[{name} {channel}] loss {l64.item():.6f} three-map vs autograd {e:.2e}; fp32 vs fp64: loss {abs(l32 - l64).item():.2e} "
          f"grad {rel_err(g32, g64):.2e}")
    assert float(g64.abs().max()) > 0
    assert e <= 1e-12
    assert abs(l32 - l64).item() <= 1e-4 * abs(l64).item() and rel_err(g32, g64) <= 1e-4
