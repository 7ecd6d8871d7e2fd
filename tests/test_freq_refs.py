"""CPU: the plain-torch restatement of the focal frequency loss (tests/freq_refs.py) differentiates to the closed form the kernels
compute, agrees with a second, independent writing of the definition, and takes its known values: Parseval at alpha = 0, the cosine
and single-pixel closed forms, and exact zeros for identical inputs."""
import pytest
import torch
import torch.nn.functional as F

import freq_refs as refs
from conftest import rel_err

ALPHAS = (0.0, 0.5, 1.0, 2.0)


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("name", list(refs.CASES))
def test_autograd_equals_closed_form_and_second_writing(name, alpha):
    x, gt = (t.double() for t in refs.case_images(name))
    l, g = refs.loss_and_grad(x, gt, alpha, torch.float64)
    gc = refs.grad_closed_form(x, gt, alpha)
    l2 = refs.freq_loss_stacked(x, gt, alpha)
    print(f"[{name} alpha={alpha}] loss {l.item():.6e} closed form vs autograd {rel_err(gc, g):.2e} second writing {abs(l2 - l).item():.2e}")
    assert l.item() > 0 and float(g.abs().max()) > 0
    assert rel_err(gc, g) <= 1e-12
    assert abs(l2 - l).item() <= 1e-12 * l.item()


@pytest.mark.parametrize("name", list(refs.CASES))
def test_alpha_zero_is_the_pixel_mse(name):
    x, gt = (t.double() for t in refs.case_images(name))
    l = refs.freq_loss(x, gt, 0.0)
    m = F.mse_loss(x, gt)
    assert abs(l - m).item() <= 1e-12 * m.item()


def test_fp32_restatement_is_close_to_fp64():
    """The fp32 evaluation stays within 1e-4 of fp64 on every case, so the 1e-3 floor of the fp64-truth rule is the binding bound of
    the GPU parity tests."""
    for name in refs.CASES:
        _, _, l32, g32, l64, g64 = refs.case(name)
        print(f"[{name}] loss {l64.item():.6e} fp32 vs fp64: loss {abs(l32 - l64).item() / l64.item():.2e} grad {rel_err(g32, g64):.2e}")
        assert abs(l32 - l64).item() <= 1e-4 * l64.item() and rel_err(g32, g64) <= 1e-4


# (H, W, u, v, the value in units of A^2): 1 where (u, v) is its own negative - DC, a Nyquist frequency on an axis with DC on the
# other, Nyquist on both - else 1/2
COSINES = [(12, 10, 3, 2, 0.5), (12, 10, 0, 0, 1.0), (12, 10, 5, 0, 1.0), (12, 10, 0, 6, 1.0), (12, 10, 5, 6, 1.0), (12, 10, 5, 2, 0.5),
           (12, 10, 3, 6, 0.5), (45, 33, 7, 11, 0.5), (45, 33, 0, 0, 1.0), (45, 33, 16, 22, 0.5), (45, 33, 0, 9, 0.5)]


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("H, W, u, v, value", COSINES)
def test_cosine_values(H, W, u, v, value, alpha):
    """d = A cos(2 pi (u x / W + v y / H)) gives A^2 / 2 per plane, and A^2 when (u, v) is its own negative, e.g. (5, 6) at 12 x 10."""
    A = 0.3
    gt = torch.zeros(1, 3, H, W, dtype=torch.float64)
    sr = gt + refs.cosine(A, u, v, H, W)
    assert refs.cosine_value(A, u, v, H, W) == value * A * A
    assert abs(refs.freq_loss(sr, gt, alpha).item() - value * A * A) <= 1e-12


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("H, W", [(1, 1), (6, 1), (12, 10), (45, 33)])
def test_single_pixel_difference(H, W, alpha):
    """A difference `a` at one pixel has a flat spectrum |D|^2 = a^2 / (HW): every weight is 1, the plane's loss a^2 / (HW)."""
    a = 0.25
    gt = torch.rand(2, 3, H, W, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    sr = gt.clone()
    sr[:, :, H // 2, W // 3] += a
    assert abs(refs.freq_loss(sr, gt, alpha).item() - a * a / (H * W)) <= 1e-12 * a * a / (H * W)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("alpha", ALPHAS)
def test_identical_inputs_give_zero_not_nan(alpha, dtype):
    x, _ = refs.images(5, 2, 12, 10)
    x = x.to(dtype)
    l, g = refs.loss_and_grad(x, x.clone(), alpha, dtype)
    assert l.item() == 0.0 and bool((g == 0).all())


@pytest.mark.parametrize("alpha", ALPHAS)
def test_one_identical_plane_contributes_nothing(alpha):
    x, gt = (t.double() for t in refs.images(6, 2, 12, 10))
    x[1, 2] = gt[1, 2]
    l, g = refs.loss_and_grad(x, gt, alpha)
    planes = [refs.freq_loss(x[b:b + 1, c:c + 1], gt[b:b + 1, c:c + 1], alpha).item() for b in range(2) for c in range(3)]
    assert planes[5] == 0.0 and min(planes[:5]) > 0
    assert abs(l.item() - sum(planes) / 6) <= 1e-12 * l.item()
    assert bool((g[1, 2] == 0).all()) and bool(torch.isfinite(g).all())
