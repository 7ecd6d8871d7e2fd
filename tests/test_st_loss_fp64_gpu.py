"""GPU: the structure-tensor loss kernels (csrc/st_loss.hip, both radius builds) held to the fp64 oracle, off the default parameters
and at the edges: normalize on / off, other taps inside each radius pair, the fused pixel + ST entry points, gS on its own, small and
ragged images, batch independence, the loss at its minimum, rank-1 structure tensors, non-finite inputs and unbuilt radii.

fp64-truth rule (conftest): loss   |hip - l64| <= max(1e-3 |l64|, 3 |l32 - l64|)
                            grads  rel_err(hip, g64) <= max(1e-3, 3 rel_err(g32, g64))
where l32 / g32 come from the fp32 oracle (the reference's arithmetic) and l64 / g64 from the same oracle in fp64.  Every case proves
from the fp64 oracle that it is not vacuous.  Run with -s for the measured errors."""
import pytest
import torch
import torch.nn.functional as F

import st_checks
from conftest import rel_err
from st_checks import BUILDS, UP, radius_of
from st_checks import check_loss as _check
from st_checks import frac_l2_above_1 as _frac_l2_above_1
from st_checks import images as _images
from st_checks import loss_hip as _hip
from st_checks import loss_oracle as _oracle

pytestmark = pytest.mark.gpu

PARAMS = [(0.5, 2.0), (0.4, 1.9), (0.6, 2.1), (1.0, 2.5), (0.9, 2.4), (1.1, 2.6)]


def test_param_grid_covers_both_builds():
    assert {(radius_of(s), radius_of(r)) for s, r in PARAMS} == {(2, 8), (4, 10)}
    assert {(radius_of(s), radius_of(r)) for s, r in BUILDS.values()} == set(BUILDS) == {(2, 8), (4, 10)}


# ------------------------------------------------------------------------------------------------ A. parameter space
@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("sigma, rho", PARAMS)
def test_st_params_vs_fp64(sigma, rho, norm):
    """normalize=False on [0, 1] images is degenerate (every eigenvalue of adj(S1) S2 is below 1): those inputs are on the 0..255
    scale."""
    x, gt = _images(int(sigma * 100 + rho * 10) + norm, 2, 48, 40, scale=1.0 if norm else 255.0)
    frac = _frac_l2_above_1(x, gt, sigma, rho, norm)
    assert frac >= 0.1, f"vacuous case: only {frac:.1%} of the pixels have l2 > 1"
    _check(f"A sigma={sigma} rho={rho} radii={radius_of(sigma), radius_of(rho)} normalize={norm} l2>1 {frac:.0%}",
           _hip(x, gt, sigma, rho, norm), _oracle(x, gt, sigma, rho, norm))


# ------------------------------------------------------------------------------------------------ B. fused pixel + ST entry points
@pytest.mark.parametrize("pix", ["mse", "l1"])
@pytest.mark.parametrize("sigma, rho, norm", [(1.0, 2.5, True), (0.5, 2.0, False), (1.0, 2.5, False)])
def test_criterion_sum_fused_pair(monkeypatch, pix, sigma, rho, norm):
    """criterion_sum with one pixel and one ST term (the training engine's path) runs sst_st_pixel_loss_fwd / _bwd; the four-launch
    form (FUSE_PIXEL_INTO_ST off) and the fp64 oracle agree with it."""
    from oracle import st as ost
    from srganst import loss as sl
    scale = 1.0 if norm else 255.0
    x, gt = _images(11 + len(pix) + norm, 2, 40, 72, scale=scale)
    crit = F.mse_loss if pix == "mse" else F.l1_loss
    w_st = 1 / 3
    w_pix = w_st * float(ost.st_loss(x, gt, sigma, rho, norm) / crit(x, gt))      # both terms carry the same weight in the total

    def run(fused):
        monkeypatch.setattr(sl, "FUSE_PIXEL_INTO_ST", fused)
        terms = [sl.StructureTensorLoss(sigma, rho, norm), sl.MSELoss() if pix == "mse" else sl.L1Loss()]
        xg = x.cuda().requires_grad_(True)
        total, weighted = sl.criterion_sum(xg, gt.cuda(), terms, [w_st, w_pix])
        (gx,) = torch.autograd.grad(total * UP, xg)
        torch.cuda.synchronize()
        return total.detach().cpu().double(), weighted.cpu(), gx.cpu().double() / UP

    def oracle(dtype):
        xo = x.to(dtype).requires_grad_(True)
        total = w_st * ost.st_loss(xo, gt.to(dtype), sigma, rho, norm) + w_pix * crit(xo, gt.to(dtype))
        (gx,) = torch.autograd.grad(total, xo)
        return total.detach().double(), gx.double()

    tf, wf, gf = run(True)
    tu, wu, gu = run(False)
    assert torch.equal(wf[0], wu[0]), (wf, wu)                       # the ST value is the same kernel's
    assert abs(tf - tu).item() <= 1e-6 * abs(tu).item() and rel_err(gf, gu) <= 1e-6, (tf, tu, rel_err(gf, gu))
    (l32, g32), (l64, g64) = oracle(torch.float32), oracle(torch.float64)
    _check(f"B fused {pix} sigma={sigma} rho={rho} normalize={norm}", (tf, gf), (l32, g32, l64, g64))


# ------------------------------------------------------------------------------------------------ C. gS on its own
@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("radii", list(BUILDS))
def test_gs_pointwise_vs_fp64(radii, norm):
    """gS = d(per-pixel distance) / d(Jxx, Jyy, Jxy of sr) straight from sst_st_loss_fwd, against fp64 autograd of the oracle's
    pointwise math (normalize, inverse, eigenvalues, distance) on the fp64 structure tensors; yardstick: the same autograd in fp32."""
    import ctypes
    from srganst import _abi
    sigma, rho = BUILDS[radii]
    B, H, W = 2, 45, 38
    x, gt = _images(23 + norm + radii[0], B, H, W, scale=1.0 if norm else 255.0)
    lib = _abi.lib()
    n = ctypes.c_int64()
    _abi.check(lib.sst_st_loss_workspace(B, H, W, ctypes.byref(n)), "sst_st_loss_workspace")
    xd, gd = x.cuda(), gt.cuda()
    loss = torch.empty((), device="cuda")
    gS = torch.full_like(xd, float("nan"))
    partials = torch.empty(n.value, device="cuda")
    counter = torch.zeros(1, device="cuda", dtype=torch.int32)
    _abi.check(lib.sst_st_loss_fwd(_abi.ptr(xd), _abi.ptr(gd), _abi.ptr(loss), _abi.ptr(gS), _abi.ptr(partials), _abi.ptr(counter),
                                   B, H, W, sigma, rho, int(norm), _abi.stream_ptr()), "sst_st_loss_fwd")
    torch.cuda.synchronize()
    st_checks.check_gs(f"C gS radii={radii} normalize={norm}", x, gt, sigma, rho, norm, gS, loss)


# ------------------------------------------------------------------------------------------------ D. geometry and batch
SIZES = [1, 2, 5, 13, 31, 32, 33, 65]


@pytest.mark.parametrize("H", SIZES)
@pytest.mark.parametrize("radii", list(BUILDS))
def test_geometry(radii, H):
    """Every W in SIZES for this H: images smaller than the 14 / 10 px halo, one-pixel rows and columns, tiles partial in one
    direction only.  Tiny images can be (nearly) structureless; non-vacuity is asserted over the whole sweep of each build."""
    sigma, rho = BUILDS[radii]
    for W in SIZES:
        x, gt = _images(H * 100 + W, 2, H, W, noise=0.1)
        _check(f"D radii={radii} {H}x{W}", _hip(x, gt, sigma, rho, True), _oracle(x, gt, sigma, rho, True))
    if H >= 13:
        x, gt = _images(H * 100 + 65, 2, H, 65, noise=0.1)
        assert _frac_l2_above_1(x, gt, sigma, rho, True) >= 0.1


@pytest.mark.parametrize("radii", list(BUILDS))
def test_batch_independence(radii):
    """Five distinct images: the batched loss is the mean of the five single-image losses, and permuting the batch permutes the
    gradient bit for bit (img_off / blockIdx.z)."""
    sigma, rho = BUILDS[radii]
    st_checks.check_batch_independence(f"D batch radii={radii}", *_images(5 + radii[0], 5, 37, 70), sigma, rho)


# ------------------------------------------------------------------------------------------------ E. numerical regimes
def _rank1(seed, B, H, W):
    """sr varies along one axis only (image 0 along H, image 1 along W): det(S1) = 0 away from the border, n = 1 / sqrt(eps)."""
    gen = torch.Generator().manual_seed(seed)
    prof = F.interpolate(torch.rand(1, 3, 12, generator=gen), size=max(H, W), mode="linear", align_corners=False)[0]
    x = torch.empty(B, 3, H, W)
    x[0] = prof[:, :H, None].expand(3, H, W)
    x[1] = prof[:, None, :W].expand(3, H, W)
    return x


@pytest.mark.parametrize("regime", ["equal", "eps1e-5", "eps1e-4", "eps1e-3", "zeros-tex", "tex-zeros", "ones-ones", "ones-tex",
                                    "tex-ones", "rank1"])
@pytest.mark.parametrize("radii", list(BUILDS))
def test_numerical_regimes(radii, regime):
    """sr == gt exactly (the loss at its minimum: the fp32 oracle gets disc = 0 exactly there, so a contraction artefact in the
    kernel's 2x2 algebra fails), sr = gt + eps noise, constant images (only the zero-padded border carries structure) and rank-1
    structure tensors of sr (the gradient runs through n = 1 / sqrt(eps))."""
    from oracle import st as ost
    sigma, rho = BUILDS[radii]
    H, W = 64, 56
    x, gt = _images(3 + radii[0] + len(regime), 2, H, W)
    if regime == "equal":
        x = gt.clone()
    elif regime.startswith("eps"):
        gen = torch.Generator().manual_seed(99)
        x = gt + float(regime[3:]) * torch.randn(gt.shape, generator=gen)
    elif regime == "rank1":
        x = _rank1(41, 2, H, W)
    else:
        const = {"zeros": torch.zeros_like(gt), "ones": torch.ones_like(gt), "tex": gt}
        a, b = regime.split("-")
        x, gt = const[a].clone(), const[b].clone()
    it = ost.st_intermediates(x.double(), gt.double(), sigma, rho, True)
    S1 = it["S1"]
    det = S1[:, 0] * S1[:, 1] - S1[:, 2] ** 2
    if regime == "equal":
        assert torch.equal(x, gt)
    elif regime.startswith("eps"):
        assert float(it["d"].max()) > 10 * float(it["d"].min())
    elif regime == "rank1":
        assert float((det < 1e-14).double().mean()) > 0.5                 # n is set by eps on most pixels
    else:
        a, b = regime.split("-")
        Sc = it["S1"] if a != "tex" else it["S2"]                        # the constant image's structure tensor
        if "zeros" in (a, b):                                            # structureless: only the eps paths run
            assert float(Sc.abs().max()) == 0 and float((it["d"] - 1e-6).abs().max()) < 1e-12
        else:                                                            # structure on the zero-padded border only
            border, inner = float(Sc[..., :2, :].abs().max()), float(Sc[..., 16:-16, 16:-16].abs().max())
            assert border > 0 and inner < 1e-12 * border, (border, inner)
            assert float(it["L"][:, 1].max()) > 1 or "tex" not in (a, b)
    ref = _oracle(x, gt, sigma, rho, True)
    if regime == "rank1":
        assert float(ref[3].abs().max()) > 0
    _check(f"E radii={radii} {regime}", _hip(x, gt, sigma, rho, True), ref)


# ------------------------------------------------------------------------------------------------ F. non-finite inputs
@pytest.mark.parametrize("where", ["corner", "inside"])
@pytest.mark.parametrize("kind", ["sr-nan", "sr-posinf", "sr-neginf", "gt-nan"])
def test_non_finite_inputs(kind, where):
    """One NaN / +inf / -inf in sr, or one NaN in gt, in batch entry 1 of 3.  The loss is non-finite exactly when the fp32 oracle's
    is (torch.clamp keeps NaN: the clamps must not mask it).  The other images' gradients are bit-identical to a run without the bad
    value.  In the affected image the gradient is non-finite exactly where the oracle's is (the kernel's masked branches multiply
    0 x NaN as autograd does), and every pixel farther than 2 (R1 + R2) from the bad one (outside its receptive field through forward
    and backward) is bit-identical to the clean run."""
    x, gt = _images(77 + len(kind) + len(where), 3, 40, 44)
    yx = (0, 0) if where == "corner" else (17, 23)
    v = {"nan": float("nan"), "posinf": float("inf"), "neginf": float("-inf")}[kind.split("-")[1]]
    xb, gtb = x.clone(), gt.clone()
    (xb if kind.startswith("sr") else gtb)[1, 1, yx[0], yx[1]] = v
    st_checks.check_non_finite(f"F {kind} {where}", x, gt, xb, gtb, yx, 0.5, 2.0)


# ------------------------------------------------------------------------------------------------ G. unsupported radii
def test_unsupported_radii_raise_cleanly():
    """The reference's structure_tensor defaults (sigma 1, rho 10 -> radii 4 / 40) are not built: forward raises HipPathError
    naming the radii, and leaves nothing behind that breaks the next valid call."""
    from srganst._abi import HipPathError
    from srganst.loss import StructureTensorLoss
    x, gt = _images(5, 2, 32, 32)
    assert (radius_of(1.0), radius_of(10.0)) == (4, 40)
    with pytest.raises(HipPathError, match=r"radii \(4,40\)"):
        StructureTensorLoss(sigma=1.0, rho=10.0)(x.cuda().requires_grad_(True), gt.cuda())
    _check("G default after unsupported", _hip(x, gt, 0.5, 2.0, True), _oracle(x, gt, 0.5, 2.0, True))
