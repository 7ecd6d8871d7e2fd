"""GPU: the structure-tensor loss and maps off the two tile builds - the separable path of csrc/st_general.hip, radii up to 8 / 20 -
held to the fp64 oracle: a grid of (sigma, rho) from radii (1, 1) to the bound, normalize on / off, gS on its own, small and ragged
images, batch independence, the path forced onto the tile builds' pairs, criterion_sum, a NaN input, the maps, graph replay and the
refusal beyond the bound.

fp64-truth rule (conftest): loss   |hip - l64| <= max(1e-3 |l64|, 3 |l32 - l64|)
                            grads  rel_err(hip, g64) <= max(1e-3, 3 rel_err(g32, g64))
where l32 / g32 come from the fp32 oracle (the reference's arithmetic: tests/test_st_general.py holds it to the reference at these
radii) and l64 / g64 from the same oracle in fp64.  Every case proves from the fp64 oracle that it is not vacuous.  Run with -s for
the measured errors."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import st_checks
import term_checks
from conftest import rel_err, truth_bound
from st_checks import BUILDS, UP, radius_of
from st_checks import check_loss as _check
from st_checks import frac_l2_above_1 as _frac_l2_above_1
from st_checks import images as _images
from st_checks import loss_hip as _hip
from st_checks import loss_oracle as _oracle

pytestmark = pytest.mark.gpu

# (sigma, rho) -> radii, none of them a tile build: smallest radii, R2 < R1, the widest k next to the narrowest g, the bound, and the
# largest values that still round into it
PAIRS = {(0.3, 0.3): (1, 1), (0.35, 0.6): (1, 2), (0.35, 5.0): (1, 20), (0.5, 1.0): (2, 4), (0.7, 1.4): (3, 6), (1.0, 2.0): (4, 8),
         (1.0, 0.6): (4, 2), (1.5, 3.0): (6, 12), (2.0, 1.0): (8, 4), (2.0, 5.0): (8, 20), (2.1, 5.1): (8, 20)}


@functools.lru_cache(maxsize=None)
def _case(seed, B, H, W, sigma, rho, norm):
    """Inputs, oracle results and the non-vacuity figure of one standard case, computed once and shared (never modified)."""
    x, gt = _images(seed, B, H, W, scale=1.0 if norm else 255.0)
    return x, gt, _oracle(x, gt, sigma, rho, norm), _frac_l2_above_1(x, gt, sigma, rho, norm)


def test_pairs_are_off_the_tile_builds_and_inside_the_bound():
    from srganst.loss import st_route
    for (sigma, rho), radii in PAIRS.items():
        assert (radius_of(sigma), radius_of(rho)) == radii and radii not in BUILDS and radii[0] <= 8 and radii[1] <= 20
        assert st_route(sigma, rho) == (True, radii)
    assert {(radius_of(s), radius_of(r)) for s, r in BUILDS.values()} == set(BUILDS)


# ------------------------------------------------------------------------------------------------ A. parameter space
@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("sigma, rho", list(PAIRS))
def test_st_params_vs_fp64(sigma, rho, norm):
    """normalize=False on [0, 1] images is degenerate (every eigenvalue of adj(S1) S2 is below 1): those inputs are on the 0..255
    scale."""
    x, gt, ref, frac = _case(int(sigma * 100 + rho * 10) + norm, 2, 48, 40, sigma, rho, norm)
    assert frac >= 0.1, f"vacuous case: only {frac:.1%} of the pixels have l2 > 1"
    _check(f"A sigma={sigma} rho={rho} radii={PAIRS[sigma, rho]} normalize={norm} l2>1 {frac:.0%}", _hip(x, gt, sigma, rho, norm), ref)


# ------------------------------------------------------------------------------------------------ B. gS on its own
@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("sigma, rho", [(1.0, 2.0), (2.0, 5.0)])
def test_gs_pointwise_vs_fp64(sigma, rho, norm):
    """gS = d(per-pixel distance) / d(Jxx, Jyy, Jxy of sr) straight from sst_st_general_fwd, against fp64 autograd of the oracle's
    pointwise math (normalize, inverse, eigenvalues, distance) on the fp64 structure tensors; yardstick: the same autograd in fp32.
    The saved planes are Ix, Iy of sr."""
    from oracle import st as ost
    from srganst import _abi
    B, H, W = 2, 45, 38
    x, gt = _images(23 + norm + radius_of(sigma), B, H, W, scale=1.0 if norm else 255.0)
    lib = _abi.lib()
    ns, nv, npart = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    _abi.check(lib.sst_st_general_workspace(B, H, W, ctypes.byref(ns), ctypes.byref(nv), ctypes.byref(npart)), "sst_st_general_workspace")
    xd, gd = x.cuda(), gt.cuda()
    loss = torch.empty((), device="cuda")
    gS = torch.full_like(xd, float("nan"))
    saved = torch.full((nv.value,), float("nan"), device="cuda")
    scratch = torch.empty(ns.value, device="cuda")
    partials = torch.empty(npart.value, device="cuda")
    counter = torch.zeros(1, device="cuda", dtype=torch.int32)
    _abi.check(lib.sst_st_general_fwd(_abi.ptr(xd), _abi.ptr(gd), _abi.ptr(loss), _abi.ptr(gS), _abi.ptr(saved), _abi.ptr(scratch),
                                      _abi.ptr(partials), _abi.ptr(counter), B, H, W, sigma, rho, int(norm), _abi.stream_ptr()),
               "sst_st_general_fwd")
    torch.cuda.synchronize()
    assert counter.item() == 0                                          # the ticket counter re-armed itself

    def grads(dtype):                                                    # Ix, Iy of sr: utils.py:219-222
        im = ost.grayscale(x.to(dtype))
        g, dg = ost.gaussian_kernel(sigma, also_dg=True, dtype=dtype)
        ix = F.conv2d(F.conv2d(im, dg.reshape(1, 1, -1, 1), padding="same"), g.reshape(1, 1, 1, -1), padding="same")
        iy = F.conv2d(F.conv2d(im, g.reshape(1, 1, -1, 1), padding="same"), dg.reshape(1, 1, 1, -1), padding="same")
        return torch.stack((ix[:, 0], iy[:, 0]))

    st_checks.check_gs(f"B gS sigma={sigma} rho={rho} normalize={norm}", x, gt, sigma, rho, norm, gS, loss)
    e_i, b_i = rel_err(saved.cpu().reshape(2, B, H, W), grads(torch.float64)), truth_bound(grads(torch.float32), grads(torch.float64))
    print(f"[B gS sigma={sigma} rho={rho} normalize={norm}] saved Ix, Iy {e_i:.3e} <= {b_i:.3e}")
    assert bool(torch.isfinite(saved).all())
    assert e_i <= b_i, (e_i, b_i)


# ------------------------------------------------------------------------------------------------ C. geometry
SIZES = [1, 2, 5, 13, 31, 32, 33, 65]


@pytest.mark.parametrize("H", SIZES)
@pytest.mark.parametrize("sigma, rho", [(2.0, 5.0), (0.35, 0.6)])
def test_geometry(sigma, rho, H):
    """Every W in SIZES for this H: images smaller than the 28 px reach of radii (8, 20), one-pixel rows and columns, strips partial
    in one direction only.  Tiny images can be (nearly) structureless; non-vacuity is asserted over the whole sweep of each pair."""
    for W in SIZES:
        x, gt = _images(H * 100 + W, 2, H, W, noise=0.1)
        _check(f"C sigma={sigma} rho={rho} {H}x{W}", _hip(x, gt, sigma, rho, True), _oracle(x, gt, sigma, rho, True))
    if H >= 13:
        x, gt = _images(H * 100 + 65, 2, H, 65, noise=0.1)
        assert _frac_l2_above_1(x, gt, sigma, rho, True) >= 0.1


# ------------------------------------------------------------------------------------------------ D. batch independence
def test_batch_independence():
    """Five distinct images: the batched loss is the mean of the five single-image losses, and permuting the batch permutes the
    gradient bit for bit (the plane index of every pass)."""
    sigma, rho = 1.0, 2.0
    st_checks.check_batch_independence("D batch", *_images(9, 5, 37, 70), sigma, rho)


# ------------------------------------------------------------------------------------------------ E. forced onto the tile builds' pairs
@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("radii", list(BUILDS))
def test_forced_general_path_against_the_tile_path(monkeypatch, radii, norm):
    """ST_FORCE_GENERAL sends a built pair down the general path: both paths obey the truth rule and agree with each other within
    it.  With the switch off the pair runs the tile kernels, launches and bits of a plain call."""
    from srganst import loss as sl
    from srganst import ops
    sigma, rho = BUILDS[radii]
    x, gt, ref, frac = _case(31 + radii[0] + norm, 2, 48, 40, sigma, rho, norm)
    assert frac >= 0.1

    def traced(force):
        monkeypatch.setattr(sl, "ST_FORCE_GENERAL", force)
        monkeypatch.setattr(ops, "TRACE_HBM", {})
        out = _hip(x, gt, sigma, rho, norm)
        return out, sorted(ops.TRACE_HBM)

    assert sl.ST_FORCE_GENERAL is False
    plain = _hip(x, gt, sigma, rho, norm)
    tile, tile_launches = traced(False)
    general, general_launches = traced(True)
    again, again_launches = traced(False)
    # (the tile backward has one launch site since the term protocol, and it registers like every other criterion launch)
    assert tile_launches == again_launches == ["st_loss_bwd_kernel", "st_loss_fwd_kernel"]
    assert general_launches == ["stg_hadj_out_kernel", "stg_loss_fwd_kernel"]
    for other in (tile, again):
        assert torch.equal(other[0], plain[0]) and torch.equal(other[1], plain[1])
    _check(f"E tile radii={radii} normalize={norm}", tile, ref)
    _check(f"E general radii={radii} normalize={norm}", general, ref)
    e, b = rel_err(general[1], tile[1]), truth_bound(ref[1], ref[3])
    print(f"[E radii={radii} normalize={norm}] general vs tile: grad rel err {e:.3e} <= {b:.3e}, "
          f"loss {general[0].item():.9e} vs {tile[0].item():.9e}")
    assert e <= b, (e, b)


# ------------------------------------------------------------------------------------------------ F. criterion_sum
@pytest.mark.parametrize("pix", ["mse", "l1"])
@pytest.mark.parametrize("st_first", [True, False])
def test_criterion_sum_general_route(pix, st_first):
    """criterion_sum with one pixel and one ST term off the tile builds: the two terms run unfused and accumulate into one d(sr),
    in either order; total and gradient against the oracle's sum, the weighted ST value against the stand-alone criterion."""
    from oracle import st as ost
    from srganst import loss as sl
    from srganst import ops
    sigma, rho, norm = 1.0, 2.0, True
    x, gt = _images(11 + len(pix), 2, 40, 72)
    assert _frac_l2_above_1(x, gt, sigma, rho, norm) >= 0.1
    crit = F.mse_loss if pix == "mse" else F.l1_loss
    w_st = 1 / 3
    w_pix = w_st * float(ost.st_loss(x, gt, sigma, rho, norm) / crit(x, gt))      # both terms carry the same weight in the total
    st_term, pix_term = sl.StructureTensorLoss(sigma, rho, norm), sl.MSELoss() if pix == "mse" else sl.L1Loss()
    terms, weights = ([st_term, pix_term], [w_st, w_pix]) if st_first else ([pix_term, st_term], [w_pix, w_st])
    k = 0 if st_first else 1
    xg = x.cuda().requires_grad_(True)
    saved_trace, ops.TRACE_HBM = ops.TRACE_HBM, {}
    try:
        total, weighted = sl.criterion_sum(xg, gt.cuda(), terms, weights)
        (gx,) = torch.autograd.grad(total * UP, xg)
        launches = set(ops.TRACE_HBM)
    finally:
        ops.TRACE_HBM = saved_trace
    alone = sl.StructureTensorLoss(sigma, rho, norm)(x.cuda(), gt.cuda())
    torch.cuda.synchronize()
    assert {"stg_loss_fwd_kernel", "stg_hadj_out_kernel"} <= launches and not {"st_loss_fwd_kernel", "st_loss_bwd_kernel"} & launches
    assert np.float32(weighted[k].item()) == np.float32(alone.item()) * np.float32(weights[k]), (weighted, alone)

    def oracle(dtype):
        xo = x.to(dtype).requires_grad_(True)
        t = w_st * ost.st_loss(xo, gt.to(dtype), sigma, rho, norm) + w_pix * crit(xo, gt.to(dtype))
        (g,) = torch.autograd.grad(t, xo)
        return t.detach().double(), g.double()

    (l32, g32), (l64, g64) = oracle(torch.float32), oracle(torch.float64)
    _check(f"F {pix} st_first={st_first}", (total.detach().cpu().double(), gx.cpu().double() / UP), (l32, g32, l64, g64))


# ------------------------------------------------------------------------------------------------ G. a NaN input
@pytest.mark.parametrize("where", ["corner", "inside"])
def test_nan_in_sr(where):
    """One NaN in sr, in batch entry 1 of 3.  The loss is non-finite exactly when the fp32 oracle's is.  The other images' gradients
    are bit-identical to a run without the bad value.  In the affected image the gradient is non-finite exactly where the oracle's
    is, and every pixel farther than 2 (R1 + R2) from the bad one (outside its receptive field through forward and backward) is
    bit-identical to the clean run."""
    x, gt = _images(77 + len(where), 3, 64, 68)
    yx = (0, 0) if where == "corner" else (30, 33)
    xb = x.clone()
    xb[1, 1, yx[0], yx[1]] = float("nan")
    st_checks.check_non_finite(f"G {where}", x, gt, xb, gt, yx, 1.0, 2.0)


# ------------------------------------------------------------------------------------------------ H. maps
@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("sigma, rho", [(1.0, 2.0), (2.0, 5.0)])
def test_maps_vs_fp64(sigma, rho, norm):
    """The bounds of tests/test_st_maps_gpu.py:test_maps_vs_fp64 on a ragged 3 x 2-tile batch, and the per-image distances against
    the loss.  The features' 1e-12 guard must stay below half an fp32 ulp of the trace: trace >= 1e-12 / 2^-24 = 1.7e-5."""
    from srganst.loss import StructureTensorLoss
    B, H, W = 2, 70, 45
    x, gt = _images(300 + radius_of(sigma) + norm, B, H, W, scale=1.0 if norm else 255.0)
    got = st_checks.check_maps_vs_fp64(f"H sigma={sigma} rho={rho} normalize={norm} {B}x{H}x{W}", x, gt, sigma, rho, norm, min_trace=1.7e-5)
    loss = StructureTensorLoss(sigma, rho, norm)(x.cuda(), gt.cuda()).item()
    assert abs(got["distance"].mean().item() - loss) <= 1e-6 * abs(loss), (got["distance"].mean().item(), loss)


@pytest.mark.parametrize("sigma, rho", [(1.0, 2.0), (2.0, 5.0)])
def test_maps_optional_outputs_are_the_same_bits(sigma, rho):
    st_checks.check_optional_outputs_are_the_same_bits(*_images(51 + radius_of(sigma), 2, 33, 31), sigma, rho)


# ------------------------------------------------------------------------------------------------ I. graph capture
def test_graph_replay_matches_eager():
    """criterion_sum forward + backward at (1.5, 3.0), captured after one warm-up call (which allocates the criterion's workspace)
    and replayed on two different inputs copied into the static tensors: loss and gradient bits equal the eager calls' each time, so
    the ticket counter re-arms inside the graph.  Everything is launched on the capturing stream: one chain, no side streams."""
    from srganst import loss as sl
    sigma, rho = 1.5, 3.0
    inputs = [_images(seed, 2, 48, 40) for seed in (501, 502, 503)]
    assert all(_frac_l2_above_1(x, gt, sigma, rho, True) >= 0.1 for x, gt in inputs)

    def run(terms, xs, gs):
        total, weighted = sl.criterion_sum(xs, gs, terms, [1 / 3, 1.0])
        (gx,) = torch.autograd.grad(total, xs)
        return total, weighted, gx
    term_checks.graph_replay_matches_eager(lambda: [sl.StructureTensorLoss(sigma, rho), sl.MSELoss()], inputs,
                                           lambda terms, xs: term_checks.ws_ptrs(terms[0], ("general_scratch",)), run, order=(1, 2, 1))


# ------------------------------------------------------------------------------------------------ J. beyond the bound
@pytest.mark.parametrize("sigma, rho, radii", [(2.2, 2.0, (9, 8)), (1.0, 5.2, (4, 21))])
def test_radii_beyond_the_bound_raise_cleanly(sigma, rho, radii):
    from srganst import st
    from srganst._abi import HipPathError
    from srganst.loss import StructureTensorLoss
    assert (radius_of(sigma), radius_of(rho)) == radii
    x, gt, ref, _ = _case(110, 2, 48, 40, 1.0, 2.0, True)
    with pytest.raises(HipPathError, match=rf"radii \({radii[0]},{radii[1]}\) not built"):
        StructureTensorLoss(sigma, rho)(x.cuda().requires_grad_(True), gt.cuda())
    with pytest.raises(HipPathError, match=rf"radii \({radii[0]},{radii[1]}\) not built"):
        st.st_distance(x.cuda(), gt.cuda(), sigma, rho)
    _check("J (1.0, 2.0) after the refusal", _hip(x, gt, 1.0, 2.0, True), ref)
