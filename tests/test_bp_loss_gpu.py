"""GPU: BackProjectionLoss and metrics.lr_consistency (csrc/bp_loss.hip) held to the plain-torch restatement of their contract
(tests/bp_refs.py) under the fp64-truth rule, to the LR image the generator sees (Bicubic on the device), and to their geometry,
scale / accumulate, determinism, graph capture, no_grad, NaN and refusal rules; then inside WarmupEngine and TrainEngine.

fp64-truth rule (conftest): loss   |hip - l64| <= max(1e-3 |l64|, 3 |l32 - l64|)
                            grads  rel_err(hip, g64) <= max(1e-3, 3 rel_err(g32, g64)), and pointwise max|hip - g64| <= 1e-3 max|g64|
where l32 / g32 are the restatement in fp32 and l64 / g64 the same in fp64, against the same target T.

    case         B x H x W       s   LR        why it is there
    one output   2 x 4 x 4       4   1 x 1     every tap clamped
    ragged       2 x 13 x 22     4   3 x 5     H, W not multiples of s
    narrow       1 x 8 x 100     4   2 x 25
    wide         1 x 8 x 1100    4   2 x 275   several column tiles: seams in x
    medium       2 x 48 x 40     4   12 x 10
    x2           2 x 30 x 26     2   15 x 13   8 taps
    x8           1 x 64 x 40     8   8 x 5     32 taps, 18 of them on the border pixel
    crop         2 x 96 x 96     4   24 x 24   the training shape: several row bands

"l1" runs where min |D| >= 1e-5 in fp64 (tests/test_bp_refs.py asserts it for bp_refs.L1_CASES: all eight with the seeds chosen).
Run with -s for the measured errors."""
import ctypes

import pytest
import torch

import bp_refs as refs
import term_checks
from conftest import assert_fp64_truth, rel_err

pytestmark = pytest.mark.gpu

UP = 0.7                                              # non-unit upstream gradient
PAIRS = [(n, c) for n in refs.CASES for c in ("l1", "mse") if c == "mse" or n in refs.L1_CASES]


def _crit(s=4, criterion="l1", round_target=True, target="gt"):
    from srganst.loss import BackProjectionLoss
    return BackProjectionLoss(s, criterion, round_target, target=target)


def _hip(x, target, crit):
    xg = x.cuda().requires_grad_(True)
    loss = crit(xg, target.cuda())
    (gx,) = torch.autograd.grad(loss * UP, xg)
    torch.cuda.synchronize()
    return loss.detach().cpu().double(), gx.cpu().double() / UP


def _hip_bits(x, target, crit):
    """Loss and gradient as the device left them (unit upstream gradient)."""
    xg = x.cuda().requires_grad_(True)
    loss = crit(xg, target.cuda())
    (gx,) = torch.autograd.grad(loss, xg)
    torch.cuda.synchronize()
    return loss.detach().cpu(), gx.cpu()


def _down_device(x, s, round_grid=0):
    """sst_bicubic straight through the C ABI: down(x) with or without the rounding to the 1/255 grid."""
    from srganst import _abi
    from srganst.bicubic import Bicubic
    B, C, H, W = x.shape
    w0, j0, w1, j1 = Bicubic("cuda").tables_i32(H, W, 1.0 / s, x.device)
    out = torch.empty(B, C, H // s, W // s, device=x.device)
    _abi.check(_abi.lib().sst_bicubic(_abi.ptr(x), _abi.ptr(out), _abi.ptr(w0), _abi.ptr(j0), _abi.ptr(w1), _abi.ptr(j1), B * C, H, W,
                                      H // s, W // s, w0.shape[1], w1.shape[1], round_grid, _abi.stream_ptr()), "sst_bicubic")
    return out


def _raw(crit, x, gt=None, lr=None, want_saved=True, per_image=False, clamp_sr=0):
    """sst_bp_loss_fwd straight through the C ABI on device tensors -> (loss, saved, counter, per_image)."""
    from srganst import _abi
    B, _, H, W = x.shape
    ns, npart = ctypes.c_int64(), ctypes.c_int64()
    _abi.check(_abi.lib().sst_bp_loss_workspace(B, H, W, crit.scale, ctypes.byref(ns), ctypes.byref(npart)), "sst_bp_loss_workspace")
    wy, iy, wx, ix = crit._tables(x.device, H, W)[:4]
    loss = torch.empty((), device="cuda")
    saved = torch.full((ns.value,), float("nan"), device="cuda") if want_saved else None
    per = torch.empty(B, device="cuda", dtype=torch.float64) if per_image else None
    partials = torch.empty(npart.value, device="cuda")
    counter = torch.zeros(1, device="cuda", dtype=torch.int32)
    _abi.check(_abi.lib().sst_bp_loss_fwd(_abi.ptr(x), _abi.ptr(gt), _abi.ptr(lr), _abi.ptr(loss), _abi.ptr(per), _abi.ptr(saved),
                                          _abi.ptr(partials), _abi.ptr(counter), _abi.ptr(wy), _abi.ptr(iy), _abi.ptr(wx), _abi.ptr(ix), B, H, W,
                                          crit.scale, wy.shape[1], wx.shape[1], int(crit.criterion == "mse"), int(crit.round_target),
                                          clamp_sr, _abi.stream_ptr()), "sst_bp_loss_fwd")
    return loss, saved, counter, per


def _raw_bwd(crit, x, saved, dsr, scale_dev=None, scale_host=1.0, accumulate=0):
    from srganst import _abi
    B, _, H, W = x.shape
    tw_y, ti_y, tw_x, ti_x = crit._tables(x.device, H, W)[4:]
    _abi.check(_abi.lib().sst_bp_loss_bwd(_abi.ptr(saved), _abi.ptr(dsr), _abi.ptr(tw_y), _abi.ptr(ti_y), _abi.ptr(tw_x), _abi.ptr(ti_x),
                                          _abi.ptr(scale_dev), float(scale_host), int(accumulate), B, H, W, crit.scale, tw_y.shape[1],
                                          tw_x.shape[1], _abi.stream_ptr()), "sst_bp_loss_bwd")
    return dsr


def _assert_truth(tag, lh, gh, l32, g32, l64, g64):
    e_l, b_l = abs(lh - l64).item(), max(1e-3 * abs(l64).item(), 3 * abs(l32 - l64).item())
    e_p, b_p = (gh - g64).abs().max().item(), 1e-3 * g64.abs().max().item()
    print(f"[{tag}] loss {lh.item():.7e} |hip-l64| {e_l:.3e} <= {b_l:.3e} | grad rel err {rel_err(gh, g64):.3e} "
          f"(fp32 restatement {rel_err(g32, g64):.3e}) | pointwise {e_p:.3e} <= {b_p:.3e}")
    assert torch.isfinite(lh) and bool(torch.isfinite(gh).all())
    assert e_l <= b_l, f"loss |hip - fp64| = {e_l:.3e} > {b_l:.3e} (hip {lh.item():.9e}, fp64 {l64.item():.9e})"
    assert_fp64_truth(f"{tag} d(sr)", gh, g32, g64)
    assert e_p <= b_p, f"pointwise gradient error {e_p:.3e} > {b_p:.3e}"


# ------------------------------------------------------------------------------------------------ A. parity
@pytest.mark.parametrize("name, criterion", PAIRS)
def test_parity_vs_fp64(name, criterion):
    """lr mode, with the target the restatement used."""
    x, _, T, s, l32, g32, l64, g64 = refs.case(name, criterion)
    lh, gh = _hip(x, T, _crit(s, criterion, target="lr"))
    _assert_truth(f"A {name} {criterion}", lh, gh, l32, g32, l64, g64)


# ------------------------------------------------------------------------------------------------ B. gt mode
@pytest.mark.parametrize("criterion", ["l1", "mse"])
@pytest.mark.parametrize("name", list(refs.CASES))
def test_gt_mode_is_the_lr_the_generator_sees(name, criterion):
    """BackProjectionLoss(sr, gt) and the lr-mode call on Bicubic("cuda")(gt, 1 / s) - the LR batch of the device gathers - give
    equal bits of loss and gradient; so does the LR image of the host data loader."""
    from srganst.bicubic import Bicubic
    x, gt, T, s, *_ = refs.case(name, criterion)
    lr = Bicubic("cuda")(gt.cuda(), 1.0 / s)
    assert torch.equal(lr.cpu(), T)                                      # the restatement's target is that LR image too
    a = _hip_bits(x, gt, _crit(s, criterion))
    b = _hip_bits(x, lr, _crit(s, criterion, target="lr"))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert bool(torch.isfinite(a[0])) and float(a[1].abs().max()) > 0


@pytest.mark.parametrize("name", list(refs.CASES))
def test_unrounded_target_vs_fp64(name):
    x, gt, T, s, l32, g32, l64, g64 = refs.case(name, "mse", False)
    lh, gh = _hip(x, gt, _crit(s, "mse", round_target=False))
    _assert_truth(f"B {name} mse unrounded", lh, gh, l32, g32, l64, g64)
    lr_, _ = _hip(x, gt, _crit(s, "mse"))
    assert lr_.item() != lh.item()                                       # the rounding is seen


# ------------------------------------------------------------------------------------------------ C. the metric
@pytest.mark.parametrize("name", list(refs.CASES))
def test_lr_consistency_vs_fp64(name):
    from srganst.metrics import lr_consistency, lr_psnr_from_mse
    x, _, T, _, s = refs.inputs(name)
    m64 = refs.per_image_mse(x, T, s)
    D32 = refs.down(x, s) - T
    m32 = (D32 * D32).mean(dim=(1, 2, 3)).double()
    got = lr_consistency(x.cuda(), T.cuda(), s, clamp=False)
    assert got.dtype == torch.float64 and tuple(got.shape) == (x.shape[0],) and got.is_cuda and not got.requires_grad
    got = got.cpu()
    for b in range(x.shape[0]):
        e, bound = abs(got[b] - m64[b]).item(), max(1e-3 * m64[b].item(), 3 * abs(m32[b] - m64[b]).item())
        print(f"[C {name} image {b}] mse {got[b].item():.7e} |hip-fp64| {e:.3e} <= {bound:.3e} LR-PSNR {lr_psnr_from_mse(got[b]):.2f} dB")
        assert e <= bound
    assert torch.equal(lr_consistency(x.cuda(), T.cuda(), s).cpu(), got)             # sr is inside [0,1]: the clamp changes nothing


def test_lr_consistency_clamp():
    from srganst.metrics import lr_consistency, lr_psnr_from_mse
    x, _, T, _, s = refs.inputs("medium")
    wild = x * 1.6 - 0.3
    assert float(wild.min()) < -0.1 and float(wild.max()) > 1.1
    on, off = lr_consistency(wild.cuda(), T.cuda(), s, clamp=True).cpu(), lr_consistency(wild.cuda(), T.cuda(), s, clamp=False).cpu()
    m_on, m_off = refs.per_image_mse(wild.clamp(0, 1), T, s), refs.per_image_mse(wild, T, s)
    assert bool(((on - off).abs() > 1e-3 * off).all())
    assert bool(((on - m_on).abs() <= 1e-3 * m_on).all()) and bool(((off - m_off).abs() <= 1e-3 * m_off).all())
    assert lr_psnr_from_mse(0.01) == pytest.approx(20.0, abs=1e-12) and lr_psnr_from_mse(0.0) == float("inf")


# ------------------------------------------------------------------------------------------------ D. geometry
@pytest.mark.parametrize("criterion", ["l1", "mse"])
def test_batch_mean_and_transpose(criterion):
    x, _ = refs.ssim_refs.images(21, 3, 44, 70)
    x[1] = x[1] * 0.5                                  # make the images differ in more than their noise
    T = refs.on_grid(refs.down(refs.ssim_refs.images(22, 3, 44, 70)[1], 4))
    crit = _crit(4, criterion, target="lr")
    xd, Td = x.cuda(), T.cuda()
    whole = crit(xd, Td).item()
    singles = [crit(xd[i:i + 1], Td[i:i + 1]).item() for i in range(3)]
    assert len(set(singles)) == 3
    assert abs(whole - sum(singles) / 3) <= 1e-6 * abs(whole), (whole, singles)
    xt, Tt = x.transpose(2, 3).contiguous(), T.transpose(2, 3).contiguous()
    swapped = crit(xt.cuda(), Tt.cuda()).item()
    assert abs(swapped - whole) <= 1e-6 * abs(whole), (swapped, whole)
    if criterion == "mse":
        _, g = _hip(x, T, crit)
        _, gt_ = _hip(xt, Tt, crit)
        assert rel_err(gt_.transpose(2, 3), g) <= 1e-6


@pytest.mark.parametrize("name, oy, ox", [("medium", 5, 4), ("medium", 0, 9), ("wide", 1, 31), ("wide", 0, 32), ("x8", 7, 0), ("x2", 8, 12),
                                          ("ragged", 2, 4)])
@pytest.mark.parametrize("criterion", ["l1", "mse"])
def test_gradient_of_one_lr_pixel_is_its_tap_footprint(name, oy, ox, criterion):
    """lr mode with lr = down(sr) bit for bit (sst_bicubic without its rounding: the same arithmetic) except at one LR pixel of one
    plane: D is exactly 0 elsewhere, so d(sr) is zero outside that pixel's tap footprint - also across tile seams - and non-zero
    inside."""
    x, _, _, _, s = refs.inputs(name)
    B, _, H, W = x.shape
    xd = x.cuda()
    lr = _down_device(xd, s)
    crit = _crit(s, criterion, target="lr")
    assert crit(xd, lr).item() == 0.0
    lr[B - 1, 1, oy, ox] += 0.1
    loss, g = _hip_bits(x, lr, crit)
    assert loss.item() > 0
    inside = refs.footprint(H, W, s, oy, ox)
    assert int(inside.sum()) >= s * s
    assert bool((g[B - 1, 1][inside] != 0).all()) and bool((g[B - 1, 1][~inside] == 0).all())
    g[B - 1, 1] = 0
    assert bool((g == 0).all())


# ------------------------------------------------------------------------------------------------ E. scale and accumulate
@pytest.mark.parametrize("criterion", ["l1", "mse"])
def test_scale_and_accumulate(criterion):
    x, gt, T, s, *_ = refs.case("ragged", criterion)
    crit = _crit(s, criterion)
    xd, gd = x.cuda(), gt.cuda()
    loss, saved, counter, _ = _raw(crit, xd, gt=gd)
    g0 = _raw_bwd(crit, xd, saved, torch.full_like(xd, float("nan")))
    torch.cuda.synchronize()
    assert counter.item() == 0                                          # the ticket counter re-armed itself
    assert bool(torch.isfinite(saved).all())                            # every element of the saved map was written
    lh, gh = _hip(x, gt, crit)
    assert loss.item() == lh.item() and rel_err(g0.cpu(), gh) <= 1e-6   # the module runs the same entries (gh went through * UP / UP)
    prefill = torch.randn(xd.shape, generator=torch.Generator().manual_seed(5)).cuda()
    acc = _raw_bwd(crit, xd, saved, prefill.clone(), accumulate=1)
    assert torch.equal(acc, prefill + g0)                               # scale 1: exactly the accumulate=0 gradient plus the prefill
    s_dev = torch.tensor(0.7, device="cuda")
    for kw, sc in (({"scale_dev": s_dev}, 0.7), ({"scale_host": 0.25}, 0.25), ({"scale_dev": s_dev, "scale_host": 0.25}, 0.175)):
        gs = _raw_bwd(crit, xd, saved, torch.full_like(xd, float("nan")), **kw)
        assert rel_err(gs.cpu(), g0.cpu().double() * sc) <= 1e-6, kw
        accs = _raw_bwd(crit, xd, saved, prefill.clone(), accumulate=1, **kw)
        assert torch.equal(accs, prefill + gs), kw


def test_per_image_and_loss_come_from_the_same_partials():
    x, gt, T, s, *_ = refs.case("crop", "mse")
    crit = _crit(s, "mse", target="lr")
    loss, _, _, per = _raw(crit, x.cuda(), lr=T.cuda(), want_saved=False, per_image=True)
    plain, _, _, _ = _raw(crit, x.cuda(), lr=T.cuda(), want_saved=False)
    assert torch.equal(loss, plain) and abs(per.mean().item() - loss.item()) <= 1e-6 * loss.item()


# ------------------------------------------------------------------------------------------------ F. determinism and capture
def test_two_eager_calls_give_equal_bits():
    cases = [(*refs.case("crop", criterion)[:2], criterion) for criterion in ("l1", "mse")]
    term_checks.two_calls_give_equal_bits([lambda c=c: _hip_bits(c[0], c[1], _crit(4, c[2])) for c in cases])


@pytest.mark.parametrize("criterion", ["l1", "mse"])
def test_graph_replay_matches_eager(criterion):
    """The warm-up call builds the criterion's tables as well: they do not move either, and there is one set of them."""
    B, H, W = 2, 48, 40
    inputs = [refs.ssim_refs.images(seed, B, H, W) for seed in (501, 502, 503)]

    def pointers(crit, xs):
        return (*term_checks.ws_ptrs(crit, ("partials", "counter")), *(t.data_ptr() for t in crit._tab[(xs.device, H, W, 4)]))
    crit = term_checks.graph_replay_matches_eager(lambda: _crit(4, criterion), inputs, pointers)
    assert len(crit._tab) == 1


# ------------------------------------------------------------------------------------------------ G. no_grad
@pytest.mark.parametrize("criterion", ["l1", "mse"])
def test_no_grad_allocates_and_writes_no_saved_map(criterion, monkeypatch):
    x, gt, T, s, *_ = refs.case("crop", criterion)
    crit = _crit(s, criterion)
    term_checks.no_grad_allocates_and_writes_nothing_saved(
        monkeypatch, crit, x, gt, saved_bytes=2 * 3 * 24 * 24 * 4, kernel="bp_loss_fwd_kernel",
        raw_loss=lambda xd, gd: _raw(crit, xd, gt=gd, want_saved=False)[0])


# ------------------------------------------------------------------------------------------------ H. NaN
@pytest.mark.parametrize("criterion", ["l1", "mse"])
def test_nan_in_sr(criterion):
    x, gt, T, s, *_ = refs.case("medium", criterion)
    B, _, H, W = x.shape
    qy, qx = 30, 33
    xb = x.clone()
    xb[0, 1, qy, qx] = float("nan")
    crit = _crit(s, criterion)
    _, g = _hip_bits(x, gt, crit)
    lb, gb = _hip_bits(xb, gt, crit)                                    # the call returns
    assert bool(torch.isnan(lb))
    My, Mx = refs.matrices(H, W, s)
    hit_y, hit_x = (My[:, qy] != 0), (Mx[:, qx] != 0)                    # the LR pixels whose taps read (qy, qx)
    assert int(hit_y.sum()) == 4 and int(hit_x.sum()) == 4
    inside = ((My != 0)[hit_y].any(dim=0))[:, None] & ((Mx != 0)[hit_x].any(dim=0))[None, :]
    assert bool(torch.isnan(gb[0, 1][inside]).all())
    assert torch.equal(gb[0, 1][~inside], g[0, 1][~inside]) and torch.equal(gb[0, 0], g[0, 0]) and torch.equal(gb[0, 2], g[0, 2])
    assert torch.equal(gb[1], g[1]) and bool(torch.isfinite(g).all())


# ------------------------------------------------------------------------------------------------ I. in the engines
def test_warmup_engine_step_vs_oracle():
    """mse: the network's 1e-3 on sr would flip L1 signs.  The oracle's target is down(gt) on the 1/255 grid, fp32 at either precision."""
    term_checks.warmup_engine_step_vs_oracle(lambda: _crit(4, "mse"), "BackProjection", 0.1,
                                             lambda sr, gt: refs.bp_loss(sr, refs.on_grid(refs.down(gt.float(), 4)), 4, "mse"))


def test_warmup_engine_graph_equals_eager():
    term_checks.warmup_engine_graph_equals_eager(_crit, "BackProjection", 0.1)


def test_train_engine_graph_equals_eager():
    term_checks.train_engine_graph_equals_eager(lambda: _crit(4, "l1"), "BackProjection", 0.1)


# ------------------------------------------------------------------------------------------------ J. refusals
def test_refusals_launch_nothing(monkeypatch):
    x, gt = refs.ssim_refs.images(81, 2, 24, 24)
    xd, gd = x.cuda(), gt.cuda()
    crit, crit_lr = _crit(), _crit(target="lr")
    lr = torch.rand(2, 3, 6, 6).cuda()
    bad = {"cpu sr": (x, gd), "cpu gt": (xd, gt), "fp64": (xd.double(), gd.double()), "one channel": (xd[:, :1], gd[:, :1]),
           "H = 3": (xd[:, :, :3], gd[:, :, :3]), "W = 3": (xd[:, :, :, :3], gd[:, :, :, :3], "3x24"),      # the size is named
           "shapes differ": (xd, gd[:1])}
    bad_lr = {"gt as lr": (xd, gd), "lr 6 x 5": (xd, lr[:, :, :, :5]), "lr batch": (xd, lr[:1]), "cpu lr": (xd, lr.cpu()),
              "fp64 lr": (xd, lr.double()), "H = 3": (xd[:, :, :3], lr[:, :, :0]), "one channel": (xd, lr[:, :1])}
    term_checks.refusals_launch_nothing(                                 # accepted: the smallest size, non-contiguous views
        monkeypatch, [(crit, *pair) for pair in bad.values()] + [(crit_lr, *pair) for pair in bad_lr.values()],
        [(crit, xd[:, :, :4, :4], gd[:, :, :4, :4]), (crit_lr, xd[:, :, :4, :4], lr[:, :, :1, :1])], "bp_loss_fwd_kernel")
