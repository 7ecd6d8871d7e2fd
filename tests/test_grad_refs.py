"""CPU: the plain-torch restatements of GradientLoss and GradientVarianceLoss (tests/grad_refs.py) - their inputs stay inside
(0, 1) unclamped, no "l1" case sits within 1e-5 of the kink of |.| (fp32 arithmetic moves M by under 1e-6 at these magnitudes, so
no sign depends on the precision), autograd agrees with central finite differences in fp64, and the fp32 and fp64 evaluations agree
to 1e-5 on every case - so the 1e-3 floor of the fp64-truth rule is the binding bound of the GPU tests."""
import pytest
import torch

import grad_refs as refs
from conftest import rel_err

VARIANTS = [(op, crit) for op in ("central", "sobel") for crit in ("l1", "mse")]


@pytest.mark.parametrize("name", list(refs.GRAD_CASES) + list(refs.GV_CASES))
def test_inputs_stay_strictly_inside_the_unit_interval(name):
    seed, B, H, W = (refs.GRAD_CASES.get(name) or refs.GV_CASES[name])[:4]
    x, gt = refs.images(seed, B, H, W)
    assert x.shape == gt.shape == (B, 3, H, W)
    for t in (x, gt):
        assert 0.0 < float(t.min()) and float(t.max()) < 1.0
    assert float((x - gt).abs().min()) > 0.0                # sr and gt coincide nowhere


@pytest.mark.parametrize("operator", ["central", "sobel"])
@pytest.mark.parametrize("name", list(refs.GRAD_CASES))
def test_no_l1_case_sits_on_the_kink(name, operator):
    gap = refs.min_magnitude_gap(name, operator)
    print(f"[{name} {operator}] min |M(sr) - M(gt)| = {gap:.3e}")
    assert gap >= 1e-5


def test_operators_respond_to_the_right_axis():
    """The vertical operator responds to row-to-row change, the horizontal one to column-to-column change; zero padding shows at
    the border."""
    rows = torch.arange(5.0).view(1, 1, 5, 1).expand(1, 1, 5, 4).contiguous()
    for op, k in (("central", 2.0), ("sobel", 8.0)):
        gv, gh = refs.responses(rows, op)
        assert torch.equal(gv[0, 0, 1:4, 1:3], torch.full((3, 2), k)) and torch.equal(gh[0, 0, :, 1:3], torch.zeros(5, 2))
        gv_t, gh_t = refs.responses(rows.transpose(2, 3).contiguous(), op)
        assert torch.equal(gh_t, gv.transpose(2, 3)) and torch.equal(gv_t, gh.transpose(2, 3))
    assert refs.responses(rows, "central")[0][0, 0, 4, 0].item() == -3.0       # the row below the image counts as zero


def test_patches_start_at_the_top_left_corner_and_drop_leftovers():
    x, _ = refs.images(5, 1, 19, 43)
    vv, vh = refs.patch_variances(x.double(), 8)
    assert vv.shape == vh.shape == (1, 2 * 5)
    gv, _ = refs.responses(refs.gray(x.double()), "sobel")
    assert abs(vv[0, 6].item() - gv[0, 0, 8:16, 8:16].var(unbiased=True).item()) <= 1e-12      # patch (1, 1), row-major


@pytest.mark.parametrize("operator, criterion", VARIANTS)
def test_gradient_loss_gradcheck_fp64(operator, criterion):
    x, gt = refs.images(3, 1, 6, 7)
    xd = x.double().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: refs.gradient_loss(t, gt.double(), operator, criterion), (xd,), eps=1e-6, atol=1e-7, rtol=1e-5)


@pytest.mark.parametrize("B, H, W, patch", [(1, 7, 9, 3), (2, 5, 4, 2)])
def test_gv_loss_gradcheck_fp64(B, H, W, patch):
    x, gt = refs.images(4, B, H, W)
    xd = x.double().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: refs.gv_loss(t, gt.double(), patch), (xd,), eps=1e-6, atol=1e-7, rtol=1e-5)
    (g,) = torch.autograd.grad(refs.gv_loss(xd, gt.double(), patch), xd)
    if H % patch:                                           # leftover rows receive gradient through the taps of the patch row above
        assert float(g[:, :, (H // patch) * patch].abs().min()) > 0.0
    if H - (H // patch) * patch > 1:                        # ... but only the first of them
        assert float(g[:, :, (H // patch) * patch + 1:].abs().max()) == 0.0


def test_identical_images_have_zero_loss_and_zero_gradient():
    x, _ = refs.images(6, 2, 12, 13)
    for fn in [lambda a, b, v=v: refs.gradient_loss(a, b, *v) for v in VARIANTS] + [lambda a, b: refs.gv_loss(a, b, 4)]:
        l, g = refs.loss_and_grad(fn, x, x.clone(), torch.float32)
        assert l.item() == 0.0 and not bool(g.any())


def _agree(tag, case):
    x, gt, l32, g32, l64, g64 = case
    e_l, e_g = abs(l32 - l64).item() / abs(l64).item(), rel_err(g32, g64)
    print(f"[{tag}] loss {l64.item():.6e} fp32 vs fp64: loss {e_l:.2e} grad {e_g:.2e}")
    assert l64.item() > 0 and float(g64.abs().max()) > 0
    assert e_l <= 1e-5 and e_g <= 1e-5


@pytest.mark.parametrize("operator, criterion", VARIANTS)
@pytest.mark.parametrize("name", list(refs.GRAD_CASES))
def test_gradient_loss_fp32_agrees_with_fp64(name, operator, criterion):
    _agree(f"{name} {operator} {criterion}", refs.case(name, operator, criterion))


@pytest.mark.parametrize("name", list(refs.GV_CASES))
def test_gv_loss_fp32_agrees_with_fp64(name):
    _agree(f"gv {name}", refs.case(name))
