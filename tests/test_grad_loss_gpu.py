"""GPU: GradientLoss and GradientVarianceLoss (csrc/grad_loss.hip) held to the plain-torch restatements of their contracts
(tests/grad_refs.py) under the fp64-truth rule, and to their tie, geometry, scale / accumulate, determinism, graph capture, no_grad,
NaN and refusal rules; then inside WarmupEngine and TrainEngine.

fp64-truth rule (conftest): loss   |hip - l64| <= max(1e-3 |l64|, 3 |l32 - l64|)
                            grads  rel_err(hip, g64) <= max(1e-3, 3 rel_err(g32, g64)), and pointwise max|hip - g64| <= 1e-3 max|g64|
where l32 / g32 are the restatement in fp32 and l64 / g64 the same in fp64.

    GradientLoss, both operators and both criteria          GradientVarianceLoss
    single row   2 x 1 x 7     no row above or below        one patch    2 x 8 x 8, p = 8
    seams        2 x 33 x 65   seams at 32 and 64, 1-px     leftover     2 x 19 x 43, p = 8    leftover rows and columns
                               partial tiles                tile of 30   1 x 31 x 34, p = 3    a tile side of 30 and a seam
    medium       2 x 48 x 40                                p5           1 x 75 x 64, p = 5
    ragged       1 x 75 x 64   three tile rows              p32          1 x 64 x 40, p = 32   one patch per workgroup
                                                            p2           1 x 9 x 5, p = 2      256 patches per tile
                                                            medium       2 x 48 x 40, p = 8

Run with -s for the measured errors."""
import ctypes

import pytest
import torch

import grad_refs as refs
import term_checks
from conftest import assert_fp64_truth, rel_err

pytestmark = pytest.mark.gpu

UP = 0.7                                              # non-unit upstream gradient
VARIANTS = [(op, crit) for op in ("central", "sobel") for crit in ("l1", "mse")]
OPS, CRITS = ("central", "sobel"), ("l1", "mse")


def _grad(operator="central", criterion="l1", eps=1e-6):
    from srganst.loss import GradientLoss
    return GradientLoss(operator, criterion, eps)


def _gv(patch=8):
    from srganst.loss import GradientVarianceLoss
    return GradientVarianceLoss(patch)


def _all_criteria():
    return [_grad(*v) for v in VARIANTS] + [_gv(8), _gv(3)]


def _hip(x, gt, crit):
    xg = x.cuda().requires_grad_(True)
    loss = crit(xg, gt.cuda())
    (gx,) = torch.autograd.grad(loss * UP, xg)
    torch.cuda.synchronize()
    return loss.detach().cpu().double(), gx.cpu().double() / UP


def _raw_grad(x, gt, op, crit, eps=1e-6):
    """sst_grad_loss_fwd straight through the C ABI on device tensors -> (loss, counter)."""
    from srganst import _abi
    B, _, H, W = x.shape
    npart = ctypes.c_int64()
    _abi.check(_abi.lib().sst_grad_loss_workspace(B, H, W, ctypes.byref(npart)), "sst_grad_loss_workspace")
    loss = torch.empty((), device="cuda")
    partials = torch.empty(npart.value, device="cuda")
    counter = torch.zeros(1, device="cuda", dtype=torch.int32)
    _abi.check(_abi.lib().sst_grad_loss_fwd(_abi.ptr(x), _abi.ptr(gt), _abi.ptr(loss), _abi.ptr(partials), _abi.ptr(counter), B, H, W,
                                            OPS.index(op), CRITS.index(crit), eps, _abi.stream_ptr()), "sst_grad_loss_fwd")
    return loss, counter


def _raw_grad_bwd(x, gt, op, crit, dsr, scale_dev=None, scale_host=1.0, accumulate=0, eps=1e-6):
    from srganst import _abi
    B, _, H, W = x.shape
    _abi.check(_abi.lib().sst_grad_loss_bwd(_abi.ptr(x), _abi.ptr(gt), _abi.ptr(dsr), _abi.ptr(scale_dev), float(scale_host), int(accumulate),
                                            B, H, W, OPS.index(op), CRITS.index(crit), eps, _abi.stream_ptr()), "sst_grad_loss_bwd")
    return dsr


def _raw_gv(x, gt, patch, want_saved=True):
    """sst_gv_loss_fwd straight through the C ABI -> (loss, saved, counter)."""
    from srganst import _abi
    B, _, H, W = x.shape
    ns, npart = ctypes.c_int64(), ctypes.c_int64()
    _abi.check(_abi.lib().sst_gv_loss_workspace(B, H, W, patch, ctypes.byref(ns), ctypes.byref(npart)), "sst_gv_loss_workspace")
    loss = torch.empty((), device="cuda")
    saved = torch.full((ns.value,), float("nan"), device="cuda") if want_saved else None
    partials = torch.empty(npart.value, device="cuda")
    counter = torch.zeros(1, device="cuda", dtype=torch.int32)
    _abi.check(_abi.lib().sst_gv_loss_fwd(_abi.ptr(x), _abi.ptr(gt), _abi.ptr(loss), _abi.ptr(saved), _abi.ptr(partials), _abi.ptr(counter),
                                          B, H, W, patch, _abi.stream_ptr()), "sst_gv_loss_fwd")
    return loss, saved, counter


def _raw_gv_bwd(x, saved, patch, dsr, scale_dev=None, scale_host=1.0, accumulate=0):
    from srganst import _abi
    B, _, H, W = x.shape
    _abi.check(_abi.lib().sst_gv_loss_bwd(_abi.ptr(x), _abi.ptr(saved), _abi.ptr(dsr), _abi.ptr(scale_dev), float(scale_host), int(accumulate),
                                          B, H, W, patch, _abi.stream_ptr()), "sst_gv_loss_bwd")
    return dsr


# ------------------------------------------------------------------------------------------------ A. parity
def _parity(tag, crit, case):
    x, gt, l32, g32, l64, g64 = case
    lh, gh = _hip(x, gt, crit)
    e_l, b_l = abs(lh - l64).item(), max(1e-3 * abs(l64).item(), 3 * abs(l32 - l64).item())
    e_p, b_p = (gh - g64).abs().max().item(), 1e-3 * g64.abs().max().item()
    print(f"[A {tag}] loss {lh.item():.7e} |hip-l64| {e_l:.3e} <= {b_l:.3e} | grad rel err {rel_err(gh, g64):.3e} "
          f"(fp32 restatement {rel_err(g32, g64):.3e}) | pointwise {e_p:.3e} <= {b_p:.3e}")
    assert torch.isfinite(lh) and bool(torch.isfinite(gh).all())
    assert e_l <= b_l, f"loss |hip - fp64| = {e_l:.3e} > {b_l:.3e} (hip {lh.item():.9e}, fp64 {l64.item():.9e})"
    assert_fp64_truth(f"{tag} d(sr)", gh, g32, g64)
    assert e_p <= b_p, f"pointwise gradient error {e_p:.3e} > {b_p:.3e}"


@pytest.mark.parametrize("operator, criterion", VARIANTS)
@pytest.mark.parametrize("name", list(refs.GRAD_CASES))
def test_gradient_loss_parity_vs_fp64(name, operator, criterion):
    _parity(f"grad {name} {operator} {criterion}", _grad(operator, criterion), refs.case(name, operator, criterion))


@pytest.mark.parametrize("name", list(refs.GV_CASES))
def test_gv_loss_parity_vs_fp64(name):
    _parity(f"gv {name}", _gv(refs.GV_CASES[name][4]), refs.case(name))


def test_other_eps_vs_fp64():
    x, gt, *_ = refs.case("medium", "sobel", "l1")
    fn = lambda a, b: refs.gradient_loss(a, b, "sobel", "l1", 1e-2)
    case = (x, gt, *refs.loss_and_grad(fn, x, gt, torch.float32), *refs.loss_and_grad(fn, x, gt, torch.float64))
    assert abs(case[4] - refs.case("medium", "sobel", "l1")[4]).item() > 1e-4 * case[4].item()        # eps matters on this input
    _parity("grad medium sobel l1 eps=1e-2", _grad("sobel", "l1", 1e-2), case)


# ------------------------------------------------------------------------------------------------ B. ties
def test_identical_images_give_exactly_zero():
    x, _ = refs.images(91, 2, 33, 40)
    for crit in _all_criteria():
        l, g = _hip(x, x.clone(), crit)
        assert l.item() == 0.0 and not bool(g.any()), crit


# ------------------------------------------------------------------------------------------------ C. geometry
def test_batch_mean_and_transpose():
    x, gt = refs.images(21, 3, 45, 70)
    x[1] = gt[1] + 0.5 * (x[1] - gt[1])                # make the images differ in more than their noise
    xd, gd = x.cuda(), gt.cuda()
    xt, gtt = x.transpose(2, 3).contiguous(), gt.transpose(2, 3).contiguous()
    for crit in _all_criteria():
        whole = crit(xd, gd).item()
        singles = [crit(xd[i:i + 1], gd[i:i + 1]).item() for i in range(3)]
        assert len(set(singles)) == 3
        assert abs(whole - sum(singles) / 3) <= 1e-6 * abs(whole), (crit, whole, singles)
        lt, g_t = _hip(xt, gtt, crit)
        l, g = _hip(x, gt, crit)
        assert abs(lt - l).item() <= 1e-6 * abs(l).item(), (crit, lt, l)
        assert rel_err(g_t.transpose(2, 3), g) <= 1e-6, crit


@pytest.mark.parametrize("operator, criterion", VARIANTS)
def test_gradient_loss_gradient_is_local_to_the_5x5_neighbourhood(operator, criterion):
    """A change of sr at one value of image 0, next to a tile seam: d(sr) keeps its bits everywhere outside the pixel's 5 x 5
    neighbourhood (the forward's taps, then the adjoint's), in the other two planes and in the other image, and changes inside."""
    x, gt = refs.images(33, 2, 48, 56)
    qy, qx = 31, 33
    x2 = x.clone()
    x2[0, 1, qy, qx] = x2[0, 1, qy, qx] + 0.04
    crit = _grad(operator, criterion)
    _, g = _hip(x, gt, crit)
    _, g2 = _hip(x2, gt, crit)
    far = torch.ones(48, 56, dtype=torch.bool)
    far[qy - 2:qy + 3, qx - 2:qx + 3] = False
    assert torch.equal(g2[1], g[1])
    assert torch.equal(g2[0, 0], g[0, 0]) and torch.equal(g2[0, 2], g[0, 2])         # the planes do not mix
    assert torch.equal(g2[0, 1][far], g[0, 1][far])
    assert int((g2[0, 1] != g[0, 1]).sum()) >= 4


def _gv_reach(q, p, size):
    """The rows (columns) of the patches that meet [q-1, q+1], grown by 1 px."""
    return slice(max(0, ((q - 1) // p) * p - 1), min(size, ((q + 1) // p + 1) * p + 1))


@pytest.mark.parametrize("patch", [8, 5])
def test_gv_loss_gradient_is_local_to_the_patches_around_the_pixel(patch):
    """The same change: d(sr) keeps its bits outside the patches that meet the pixel's 3 x 3 neighbourhood, grown by 1 px, and in the
    other image; the three planes share the gray image, so all of them change inside."""
    x, gt = refs.images(34, 2, 48, 56)
    qy, qx = 20, 32                                    # on a patch boundary of p = 8, next to the tile seams of both patch sizes
    x2 = x.clone()
    x2[0, 1, qy, qx] = x2[0, 1, qy, qx] + 0.04
    _, g = _hip(x, gt, _gv(patch))
    _, g2 = _hip(x2, gt, _gv(patch))
    far = torch.ones(48, 56, dtype=torch.bool)
    far[_gv_reach(qy, patch, 48), _gv_reach(qx, patch, 56)] = False
    assert torch.equal(g2[1], g[1])
    assert torch.equal(g2[0][:, far], g[0][:, far])
    changed = (g2[0] != g[0]).all(dim=0)
    assert int(changed.sum()) >= patch * patch and not bool(changed[far].any())


def test_gv_loss_leftover_pixels_receive_gradient():
    """19 x 43 at p = 8: rows 16.., columns 40.. belong to no patch; the first leftover row and column still receive gradient through
    the Sobel taps of the patch pixels next to them, the ones behind them exactly zero."""
    x, gt, *_ = refs.case("leftover")
    _, g = _hip(x, gt, _gv(8))
    assert float(g[:, :, 16, :40].abs().min()) > 0 and float(g[:, :, :16, 40].abs().min()) > 0
    assert not bool(g[:, :, 17:].any()) and not bool(g[:, :, :, 41:].any())


# ------------------------------------------------------------------------------------------------ D. scale and accumulate
def _scale_and_accumulate(xd, g0, bwd):
    """bwd(dsr, **kw) -> dsr: the raw backward entry on the forward that gave g0 = bwd(NaN-filled buffer)."""
    assert bool(torch.isfinite(g0).all())                                # every element was written
    prefill = torch.randn(xd.shape, generator=torch.Generator().manual_seed(5)).cuda()
    acc = bwd(prefill.clone(), accumulate=1)
    assert torch.equal(acc, prefill + g0)                               # scale 1: exactly the accumulate=0 gradient plus the prefill
    s_dev = torch.tensor(0.7, device="cuda")
    for kw, s in (({"scale_dev": s_dev}, 0.7), ({"scale_host": 0.25}, 0.25), ({"scale_dev": s_dev, "scale_host": 0.25}, 0.175)):
        gs = bwd(torch.full_like(xd, float("nan")), **kw)
        assert rel_err(gs.cpu(), g0.cpu().double() * s) <= 1e-6, kw
        accs = bwd(prefill.clone(), accumulate=1, **kw)
        assert torch.equal(accs, prefill + gs), kw


@pytest.mark.parametrize("operator, criterion", VARIANTS)
def test_gradient_loss_scale_and_accumulate(operator, criterion):
    x, gt, *_ = refs.case("ragged", operator, criterion)
    xd, gd = x.cuda(), gt.cuda()
    loss, counter = _raw_grad(xd, gd, operator, criterion)
    g0 = _raw_grad_bwd(xd, gd, operator, criterion, torch.full_like(xd, float("nan")))
    torch.cuda.synchronize()
    assert counter.item() == 0                                          # the ticket counter re-armed itself
    lh, gh = _hip(x, gt, _grad(operator, criterion))
    assert loss.item() == lh.item() and rel_err(g0.cpu(), gh) <= 1e-6   # the module runs the same entries (gh went through * UP / UP)
    _scale_and_accumulate(xd, g0, lambda dsr, **kw: _raw_grad_bwd(xd, gd, operator, criterion, dsr, **kw))


@pytest.mark.parametrize("name", ["leftover", "p5"])
def test_gv_loss_scale_and_accumulate(name):
    patch = refs.GV_CASES[name][4]
    x, gt, *_ = refs.case(name)
    xd, gd = x.cuda(), gt.cuda()
    loss, saved, counter = _raw_gv(xd, gd, patch)
    g0 = _raw_gv_bwd(xd, saved, patch, torch.full_like(xd, float("nan")))
    torch.cuda.synchronize()
    assert counter.item() == 0
    assert bool(torch.isfinite(saved).all())                            # four floats of every patch were written
    lh, gh = _hip(x, gt, _gv(patch))
    assert loss.item() == lh.item() and rel_err(g0.cpu(), gh) <= 1e-6
    _scale_and_accumulate(xd, g0, lambda dsr, **kw: _raw_gv_bwd(xd, saved, patch, dsr, **kw))


# ------------------------------------------------------------------------------------------------ E. determinism and capture
def test_two_eager_calls_give_equal_bits():
    x, gt, *_ = refs.case("ragged", "sobel", "l1")
    term_checks.two_calls_give_equal_bits([lambda c=c: _hip(x, gt, c) for c in _all_criteria() + [_gv(5)]])


@pytest.mark.parametrize("make", [lambda: _grad("central", "l1"), lambda: _grad("sobel", "mse"), _gv], ids=["central-l1", "sobel-mse", "gv"])
def test_graph_replay_matches_eager(make):
    inputs = [refs.images(seed, 2, 48, 40) for seed in (501, 502, 503)]
    term_checks.graph_replay_matches_eager(make, inputs, lambda crit, xs: term_checks.ws_ptrs(crit, ("partials", "counter")))


# ------------------------------------------------------------------------------------------------ F. no_grad
def test_gradient_loss_no_grad_allocates_nothing(monkeypatch):
    """GradientLoss saves nothing either way: under no_grad not even a buffer of one plane's size is allocated."""
    term_checks.no_grad_allocates_and_writes_nothing_saved(
        monkeypatch, _grad("sobel", "l1"), *refs.images(61, 2, 96, 96), saved_bytes=96 * 96 * 4, kernel="grad_loss_fwd_kernel",
        raw_loss=lambda xd, gd: _raw_grad(xd, gd, "sobel", "l1")[0])


def test_gv_loss_no_grad_allocates_and_writes_nothing_saved(monkeypatch):
    term_checks.no_grad_allocates_and_writes_nothing_saved(
        monkeypatch, _gv(8), *refs.images(61, 2, 96, 96), saved_bytes=4 * 2 * 12 * 12 * 4, kernel="gv_loss_fwd_kernel",
        raw_loss=lambda xd, gd: _raw_gv(xd, gd, 8, want_saved=False)[0])


def test_gradient_for_gt_is_refused():
    from srganst._abi import HipPathError
    x, gt = (t.cuda() for t in refs.images(62, 1, 16, 16))
    for crit in (_grad(), _gv()):
        with pytest.raises(HipPathError, match="with respect to sr only"):
            crit(x, gt.clone().requires_grad_(True)).backward()


# ------------------------------------------------------------------------------------------------ G. NaN
@pytest.mark.parametrize("operator, criterion", VARIANTS)
def test_gradient_loss_nan_in_sr(operator, criterion):
    x, gt = refs.images(71, 2, 48, 56)
    qy, qx = 30, 33
    xb = x.clone()
    xb[0, 1, qy, qx] = float("nan")
    crit = _grad(operator, criterion)
    _, g = _hip(x, gt, crit)
    lb, gb = _hip(xb, gt, crit)                                         # the call returns
    assert bool(torch.isnan(lb)) and bool(torch.isnan(gb[0, 1, qy, qx]))
    far = torch.ones(48, 56, dtype=torch.bool)
    far[qy - 2:qy + 3, qx - 2:qx + 3] = False
    assert torch.equal(gb[0, 1][far], g[0, 1][far]) and torch.equal(gb[1], g[1])
    assert torch.equal(gb[0, 0], g[0, 0]) and torch.equal(gb[0, 2], g[0, 2])


@pytest.mark.parametrize("patch", [8, 5])
def test_gv_loss_nan_in_sr(patch):
    x, gt = refs.images(72, 2, 48, 56)
    qy, qx = 20, 32
    xb = x.clone()
    xb[0, 1, qy, qx] = float("nan")
    _, g = _hip(x, gt, _gv(patch))
    lb, gb = _hip(xb, gt, _gv(patch))
    assert bool(torch.isnan(lb)) and bool(torch.isnan(gb[0, :, qy, qx]).all())
    far = torch.ones(48, 56, dtype=torch.bool)
    far[_gv_reach(qy, patch, 48), _gv_reach(qx, patch, 56)] = False
    assert torch.equal(gb[0][:, far], g[0][:, far]) and torch.equal(gb[1], g[1])


# ------------------------------------------------------------------------------------------------ H. in the engines
ENGINE_TERMS = {"Gradient": (_grad, lambda sr, gt: refs.gradient_loss(sr, gt)), "GV": (_gv, lambda sr, gt: refs.gv_loss(sr, gt))}


@pytest.mark.parametrize("name", list(ENGINE_TERMS))
def test_warmup_engine_step_vs_oracle(name):
    make, ref = ENGINE_TERMS[name]
    term_checks.warmup_engine_step_vs_oracle(make, name, 0.1, ref)


@pytest.mark.parametrize("name", list(ENGINE_TERMS))
def test_warmup_engine_graph_equals_eager(name):
    term_checks.warmup_engine_graph_equals_eager(ENGINE_TERMS[name][0], name, 0.1)


@pytest.mark.parametrize("name", list(ENGINE_TERMS))
def test_train_engine_graph_equals_eager(name):
    term_checks.train_engine_graph_equals_eager(ENGINE_TERMS[name][0], name, 0.1)


# ------------------------------------------------------------------------------------------------ I. refusals
@pytest.mark.parametrize("which", ["grad", "gv"])
def test_refusals_launch_nothing(which, monkeypatch):
    x, gt = refs.images(81, 2, 24, 24)
    xd, gd = x.cuda(), gt.cuda()
    crit = _grad() if which == "grad" else _gv()
    bad = {"cpu sr": (x, gd), "cpu gt": (xd, gt), "fp64": (xd.double(), gd.double()), "one channel": (xd[:, :1], gd[:, :1]),
           "shapes differ": (xd, gd[:1])}
    if which == "gv":
        bad.update({"H = 7": (xd[:, :, :7], gd[:, :, :7], "below the patch size 8"), "W = 7": (xd[:, :, :, :7], gd[:, :, :, :7], "below the patch size 8")})
    side = 1 if which == "grad" else 8
    term_checks.refusals_launch_nothing(monkeypatch, [(crit, *pair) for pair in bad.values()],
                                        [(crit, xd[:, :, :side, :side], gd[:, :, :side, :side])], f"{which}_loss_fwd_kernel")
