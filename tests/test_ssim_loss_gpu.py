"""GPU: SSIMLoss (csrc/ssim_loss.hip) held to the plain-torch restatement of its contract (tests/ssim_refs.py) under the fp64-truth
rule, to the SSIM the drivers report (metrics.image_metrics_device), and to its geometry, scale / accumulate, determinism, graph
capture, no_grad, NaN and refusal rules; then inside WarmupEngine and TrainEngine.

fp64-truth rule (conftest): loss   |hip - l64| <= max(1e-3 |l64|, 3 |l32 - l64|)
                            grads  rel_err(hip, g64) <= max(1e-3, 3 rel_err(g32, g64)), and pointwise max|hip - g64| <= 1e-3 max|g64|
where l32 / g32 are the restatement in fp32 and l64 / g64 the same in fp64.

    case             B x H x W     noise   why it is there
    one window       2 x 11 x 11   0.08    a single window per plane
    narrow           2 x 12 x 43   0.08    2 x 33 outputs: a tile seam in x, a 1-column partial tile
    medium           2 x 48 x 40   0.08
    anti-correlated  3 x 45 x 33   0.3     N2 < 0 at 1 - 2 % of the positions (tests/test_ssim_refs.py asserts it)
    ragged           1 x 75 x 64   0.02    65 x 54 outputs: three tiles per axis, ragged both ways

Run with -s for the measured errors."""
import ctypes

import pytest
import torch

import ssim_refs as refs
import term_checks
from conftest import assert_fp64_truth, rel_err

pytestmark = pytest.mark.gpu

UP = 0.7                                              # non-unit upstream gradient


def _hip(x, gt, channel, crit=None):
    from srganst.loss import SSIMLoss
    crit = crit if crit is not None else SSIMLoss(channel)
    xg = x.cuda().requires_grad_(True)
    loss = crit(xg, gt.cuda())
    (gx,) = torch.autograd.grad(loss * UP, xg)
    torch.cuda.synchronize()
    return loss.detach().cpu().double(), gx.cpu().double() / UP


def _raw(x, gt, planes, want_maps=True, k1=0.01, k2=0.03):
    """sst_ssim_loss_fwd straight through the C ABI on device tensors -> (loss, maps, counter)."""
    from srganst import _abi
    B, _, H, W = x.shape
    nm, npart = ctypes.c_int64(), ctypes.c_int64()
    _abi.check(_abi.lib().sst_ssim_loss_workspace(B, H, W, planes, ctypes.byref(nm), ctypes.byref(npart)), "sst_ssim_loss_workspace")
    loss = torch.empty((), device="cuda")
    maps = torch.full((nm.value,), float("nan"), device="cuda") if want_maps else None
    partials = torch.empty(npart.value, device="cuda")
    counter = torch.zeros(1, device="cuda", dtype=torch.int32)
    _abi.check(_abi.lib().sst_ssim_loss_fwd(_abi.ptr(x), _abi.ptr(gt), _abi.ptr(loss), _abi.ptr(maps), _abi.ptr(partials), _abi.ptr(counter),
                                            B, H, W, planes, k1, k2, _abi.stream_ptr()), "sst_ssim_loss_fwd")
    return loss, maps, counter


def _raw_bwd(x, gt, maps, planes, dsr, scale_dev=None, scale_host=1.0, accumulate=0):
    from srganst import _abi
    B, _, H, W = x.shape
    _abi.check(_abi.lib().sst_ssim_loss_bwd(_abi.ptr(x), _abi.ptr(gt), _abi.ptr(maps), _abi.ptr(dsr), _abi.ptr(scale_dev), float(scale_host),
                                            int(accumulate), B, H, W, planes, _abi.stream_ptr()), "sst_ssim_loss_bwd")
    return dsr


# ------------------------------------------------------------------------------------------------ A. parity
@pytest.mark.parametrize("channel", ["y", "rgb"])
@pytest.mark.parametrize("name", list(refs.CASES))
def test_parity_vs_fp64(name, channel):
    x, gt, l32, g32, l64, g64 = refs.case(name, channel)
    lh, gh = _hip(x, gt, channel)
    e_l, b_l = abs(lh - l64).item(), max(1e-3 * abs(l64).item(), 3 * abs(l32 - l64).item())
    e_p, b_p = (gh - g64).abs().max().item(), 1e-3 * g64.abs().max().item()
    print(f"[A {name} {channel}] loss {lh.item():.7f} |hip-l64| {e_l:.3e} <= {b_l:.3e} | grad rel err {rel_err(gh, g64):.3e} "
          f"(fp32 restatement {rel_err(g32, g64):.3e}) | pointwise {e_p:.3e} <= {b_p:.3e}")
    assert torch.isfinite(lh) and bool(torch.isfinite(gh).all())
    assert e_l <= b_l, f"loss |hip - fp64| = {e_l:.3e} > {b_l:.3e} (hip {lh.item():.9e}, fp64 {l64.item():.9e})"
    assert_fp64_truth(f"{name} {channel} d(sr)", gh, g32, g64)
    assert e_p <= b_p, f"pointwise gradient error {e_p:.3e} > {b_p:.3e}"


@pytest.mark.parametrize("k1, k2", [(0.02, 0.05), (0.001, 0.2)])
def test_other_constants_vs_fp64(k1, k2):
    from srganst.loss import SSIMLoss
    x, gt, *_ = refs.case("medium", "y")
    l32, g32 = refs.loss_and_grad(x, gt, "y", torch.float32, k1, k2)
    l64, g64 = refs.loss_and_grad(x, gt, "y", torch.float64, k1, k2)
    lh, gh = _hip(x, gt, "y", SSIMLoss("y", k1, k2))
    assert abs(l64 - refs.case("medium", "y")[4]).item() > 1e-2        # the constants matter on this input
    assert abs(lh - l64).item() <= max(1e-3 * abs(l64).item(), 3 * abs(l32 - l64).item())
    assert_fp64_truth(f"k1={k1} k2={k2} d(sr)", gh, g32, g64)


# ------------------------------------------------------------------------------------------------ B. the metric the drivers report
@pytest.mark.parametrize("seed, B, H, W", [(9, 1, 60, 52), (10, 2, 96, 96)])
def test_one_minus_loss_is_the_validation_ssim(seed, B, H, W):
    from srganst.loss import SSIMLoss
    from srganst.metrics import image_metrics_device
    x, gt = (refs.on_grid(t).cuda() for t in refs.images(seed, B, H, W))
    ssim = image_metrics_device(x, gt)[:, 1].cpu()
    crit = SSIMLoss("y")
    for i in range(B):
        mine = 1.0 - crit(x[i:i + 1], gt[i:i + 1]).item()
        print(f"[B {H}x{W} image {i}] 1 - loss {mine:.8f} metric {ssim[i].item():.8f}")
        assert 0 < ssim[i].item() < 0.999
        assert abs(mine - ssim[i].item()) <= 1e-3 * ssim[i].item()


# ------------------------------------------------------------------------------------------------ C. geometry
@pytest.mark.parametrize("channel", ["y", "rgb"])
def test_batch_mean_and_transpose(channel):
    from srganst.loss import SSIMLoss
    x, gt = refs.images(21, 3, 45, 70)
    x[1] = x[1] * 0.5                                  # make the images differ in more than their noise
    crit = SSIMLoss(channel)
    xd, gd = x.cuda(), gt.cuda()
    whole = crit(xd, gd).item()
    singles = [crit(xd[i:i + 1], gd[i:i + 1]).item() for i in range(3)]
    assert len(set(singles)) == 3
    assert abs(whole - sum(singles) / 3) <= 1e-6 * abs(whole), (whole, singles)
    swapped = crit(xd.transpose(2, 3).contiguous(), gd.transpose(2, 3).contiguous()).item()
    assert abs(swapped - whole) <= 1e-6 * abs(whole), (swapped, whole)
    lt, gt_ = _hip(x.transpose(2, 3).contiguous(), gt.transpose(2, 3).contiguous(), channel)
    _, g = _hip(x, gt, channel)
    assert rel_err(gt_.transpose(2, 3), g) <= 1e-6


@pytest.mark.parametrize("channel", ["y", "rgb"])
def test_gradient_is_local_to_the_21x21_neighbourhood(channel):
    """A change of sr at one pixel (one channel) of image 0, next to a tile seam: d(sr) keeps its bits everywhere outside the
    pixel's 21 x 21 neighbourhood (forward window, then the backward's) and in the other image, and changes inside."""
    x, gt = refs.images(33, 2, 48, 56)
    qy, qx = 20, 33
    x2 = x.clone()
    x2[0, 1, qy, qx] = (x2[0, 1, qy, qx] + 0.25) % 1.0
    _, g = _hip(x, gt, channel)
    _, g2 = _hip(x2, gt, channel)
    far = torch.ones(48, 56, dtype=torch.bool)
    far[qy - 10:qy + 11, qx - 10:qx + 11] = False
    assert torch.equal(g2[1], g[1])
    assert torch.equal(g2[0][:, far], g[0][:, far])
    changed = (g2[0] != g[0]).any(dim=0)
    assert int(changed.sum()) > 200 and not bool(changed[far].any())
    if channel == "rgb":                               # the planes do not mix
        assert torch.equal(g2[0, 0], g[0, 0]) and torch.equal(g2[0, 2], g[0, 2])


# ------------------------------------------------------------------------------------------------ D. scale and accumulate
@pytest.mark.parametrize("planes", [1, 3])
def test_scale_and_accumulate(planes):
    channel = "y" if planes == 1 else "rgb"
    x, gt, *_ = refs.case("ragged", channel)
    xd, gd = x.cuda(), gt.cuda()
    loss, maps, counter = _raw(xd, gd, planes)
    g0 = _raw_bwd(xd, gd, maps, planes, torch.full_like(xd, float("nan")))
    torch.cuda.synchronize()
    assert counter.item() == 0                                          # the ticket counter re-armed itself
    assert bool(torch.isfinite(maps).all())                             # every map element was written
    lh, gh = _hip(x, gt, channel)
    assert loss.item() == lh.item() and rel_err(g0.cpu(), gh) <= 1e-6   # the module runs the same entries (gh went through * UP / UP)
    prefill = torch.randn(xd.shape, generator=torch.Generator().manual_seed(5)).cuda()
    acc = _raw_bwd(xd, gd, maps, planes, prefill.clone(), accumulate=1)
    assert torch.equal(acc, prefill + g0)                               # scale 1: exactly the accumulate=0 gradient plus the prefill
    s_dev = torch.tensor(0.7, device="cuda")
    for kw, s in (({"scale_dev": s_dev}, 0.7), ({"scale_host": 0.25}, 0.25), ({"scale_dev": s_dev, "scale_host": 0.25}, 0.175)):
        gs = _raw_bwd(xd, gd, maps, planes, torch.full_like(xd, float("nan")), **kw)
        assert rel_err(gs.cpu(), g0.cpu().double() * s) <= 1e-6, kw
        accs = _raw_bwd(xd, gd, maps, planes, prefill.clone(), accumulate=1, **kw)
        assert torch.equal(accs, prefill + gs), kw


# ------------------------------------------------------------------------------------------------ E. determinism and capture
def test_two_eager_calls_give_equal_bits():
    cases = [(*refs.case("ragged", channel)[:2], channel) for channel in ("y", "rgb")]
    term_checks.two_calls_give_equal_bits([lambda c=c: _hip(*c) for c in cases])


@pytest.mark.parametrize("channel", ["y", "rgb"])
def test_graph_replay_matches_eager(channel):
    from srganst.loss import SSIMLoss
    inputs = [refs.images(seed, 2, 48, 40) for seed in (501, 502, 503)]
    term_checks.graph_replay_matches_eager(lambda: SSIMLoss(channel), inputs, lambda crit, xs: term_checks.ws_ptrs(crit, ("partials", "counter")))


# ------------------------------------------------------------------------------------------------ F. no_grad
@pytest.mark.parametrize("channel", ["y", "rgb"])
def test_no_grad_allocates_and_writes_no_maps(channel, monkeypatch):
    from srganst.loss import SSIMLoss
    planes = 1 if channel == "y" else 3
    term_checks.no_grad_allocates_and_writes_nothing_saved(
        monkeypatch, SSIMLoss(channel), *refs.images(61, 2, 96, 96), saved_bytes=2 * planes * 86 * 86 * 3 * 4, kernel="ssim_loss_fwd_kernel",
        raw_loss=lambda xd, gd: _raw(xd, gd, planes, want_maps=False)[0])


# ------------------------------------------------------------------------------------------------ G. NaN
@pytest.mark.parametrize("channel", ["y", "rgb"])
def test_nan_in_sr(channel):
    x, gt = refs.images(71, 2, 48, 56)
    qy, qx = 30, 33
    xb = x.clone()
    xb[0, 1, qy, qx] = float("nan")
    _, g = _hip(x, gt, channel)
    lb, gb = _hip(xb, gt, channel)                                      # the call returns
    assert bool(torch.isnan(lb))
    assert bool(torch.isnan(gb[0, 1, qy, qx])) and bool(torch.isnan(gb[0, 1, qy - 10:qy + 11, qx - 10:qx + 11]).all())
    far = torch.ones(48, 56, dtype=torch.bool)
    far[qy - 10:qy + 11, qx - 10:qx + 11] = False
    assert torch.equal(gb[0][:, far], g[0][:, far]) and torch.equal(gb[1], g[1])


# ------------------------------------------------------------------------------------------------ H. in the engines
def _ssim():
    from srganst.loss import SSIMLoss
    return SSIMLoss()


def test_warmup_engine_step_vs_oracle():
    term_checks.warmup_engine_step_vs_oracle(_ssim, "SSIM", 0.1, lambda sr, gt: refs.ssim_loss(sr, gt, "y"))


def test_warmup_engine_graph_equals_eager():
    term_checks.warmup_engine_graph_equals_eager(_ssim, "SSIM", 0.1)


def test_train_engine_graph_equals_eager():
    term_checks.train_engine_graph_equals_eager(_ssim, "SSIM", 0.1)


# ------------------------------------------------------------------------------------------------ I. refusals
def test_refusals_launch_nothing(monkeypatch):
    x, gt = refs.images(81, 2, 24, 24)
    xd, gd = x.cuda(), gt.cuda()
    crit = _ssim()
    bad = {"cpu sr": (x, gd), "cpu gt": (xd, gt), "fp64": (xd.double(), gd.double()), "one channel": (xd[:, :1], gd[:, :1]),
           "H = 10": (xd[:, :, :10], gd[:, :, :10]), "W = 10": (xd[:, :, :, :10], gd[:, :, :, :10]), "shapes differ": (xd, gd[:1])}
    term_checks.refusals_launch_nothing(monkeypatch, [(crit, a, b) for a, b in bad.values()],
                                        [(crit, xd[:, :, :11, :11], gd[:, :, :11, :11])], "ssim_loss_fwd_kernel")
