"""GPU: FocalFrequencyLoss (csrc/freq_loss.hip) held to the plain-torch restatement of its contract (tests/freq_refs.py) under the
fp64-truth rule, to its closed forms (the check of the half spectrum's multiplicities), to its structure, scale / accumulate,
determinism, graph capture, no_grad, NaN and refusal rules; then inside WarmupEngine and TrainEngine.

fp64-truth rule (conftest): loss   |hip - l64| <= max(1e-3 |l64|, 3 |l32 - l64|)
                            grads  rel_err(hip, g64) <= max(1e-3, 3 rel_err(g32, g64)), and pointwise max|hip - g64| <= 1e-3 max|g64|
where l32 / g32 are the restatement in fp32 and l64 / g64 the same in fp64.

    case       B x H x W      why it is there
    pixel      2 x 1 x 1      smallest accepted size
    row        1 x 1 x 7      single row
    column     1 x 6 x 1      single column
    even       2 x 12 x 10    Nyquist column and row
    odd        2 x 45 x 33    no Nyquist, nothing a multiple of a block
    mixed      1 x 48 x 37    even H, odd W
    ragged     1 x 75 x 64
    crop       2 x 96 x 96    the training crop
    tall       1 x 130 x 18   crosses the 128-element staging chunk on one axis
    longest    1 x 512 x 5    the bound, cheaply
    dominant   2 x 40 x 36    d = 0.2 + 0.01 randn: DC carries the maximum, the weights span many decades

Closed forms and invariances on the device are held to 1e-5 relative: the transforms are fp32 sums of at most 96 terms there
(error about sqrt(N) 2^-24 per coefficient, twice that in its square), the bound the issue sets for alpha = 0 against MSELoss.

Run with -s for the measured errors."""
import ctypes

import pytest
import torch

import freq_refs as refs
import term_checks
from conftest import assert_fp64_truth, rel_err

pytestmark = pytest.mark.gpu

UP = 0.7                                              # non-unit upstream gradient
CLOSED = 1e-5                                         # see the module docstring


def _hip(x, gt, alpha=1.0, crit=None):
    from srganst.loss import FocalFrequencyLoss
    crit = crit if crit is not None else FocalFrequencyLoss(alpha)
    xg = x.cuda().requires_grad_(True)
    loss = crit(xg, gt.cuda())
    (gx,) = torch.autograd.grad(loss * UP, xg)
    torch.cuda.synchronize()
    return loss.detach().cpu().double(), gx.cpu().double() / UP


def _loss(x, gt, alpha=1.0):
    from srganst.loss import FocalFrequencyLoss
    with torch.no_grad():
        return FocalFrequencyLoss(alpha)(x.float().cuda(), gt.float().cuda()).item()


def _raw(x, gt, alpha=1.0, want_saved=True):
    """sst_freq_loss_fwd straight through the C ABI on device tensors -> (loss, saved, scratch, counter)."""
    from srganst import _abi
    B, _, H, W = x.shape
    ns, nscr, npart = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    _abi.check(_abi.lib().sst_freq_loss_workspace(B, H, W, ctypes.byref(ns), ctypes.byref(nscr), ctypes.byref(npart)), "sst_freq_loss_workspace")
    loss = torch.empty((), device="cuda")
    saved = torch.full((ns.value,), float("nan"), device="cuda") if want_saved else None
    scratch = torch.empty(nscr.value, device="cuda")
    partials = torch.empty(npart.value, device="cuda")
    counter = torch.zeros(1, device="cuda", dtype=torch.int32)
    _abi.check(_abi.lib().sst_freq_loss_fwd(_abi.ptr(x), _abi.ptr(gt), _abi.ptr(loss), _abi.ptr(saved), _abi.ptr(scratch), _abi.ptr(partials),
                                            _abi.ptr(counter), B, H, W, float(alpha), _abi.stream_ptr()), "sst_freq_loss_fwd")
    return loss, saved, scratch, counter


def _raw_bwd(shape, saved, scratch, dsr, scale_dev=None, scale_host=1.0, accumulate=0):
    from srganst import _abi
    B, _, H, W = shape
    _abi.check(_abi.lib().sst_freq_loss_bwd(_abi.ptr(saved), _abi.ptr(dsr), _abi.ptr(scratch), _abi.ptr(scale_dev), float(scale_host),
                                            int(accumulate), B, H, W, _abi.stream_ptr()), "sst_freq_loss_bwd")
    return dsr


# ------------------------------------------------------------------------------------------------ A. parity
PARITY = [(name, 1.0) for name in refs.CASES] + [(name, a) for name in ("odd", "crop") for a in (0.5, 2.0)]


@pytest.mark.parametrize("name, alpha", PARITY)
def test_parity_vs_fp64(name, alpha):
    x, gt, l32, g32, l64, g64 = refs.case(name, alpha)
    lh, gh = _hip(x, gt, alpha)
    e_l, b_l = abs(lh - l64).item(), max(1e-3 * abs(l64).item(), 3 * abs(l32 - l64).item())
    e_p, b_p = (gh - g64).abs().max().item(), 1e-3 * g64.abs().max().item()
    print(f"[A {name} alpha={alpha}] loss {lh.item():.7e} |hip-l64| {e_l:.3e} <= {b_l:.3e} | grad rel err {rel_err(gh, g64):.3e} "
          f"(fp32 restatement {rel_err(g32, g64):.3e}) | pointwise {e_p:.3e} <= {b_p:.3e}")
    assert torch.isfinite(lh) and bool(torch.isfinite(gh).all())
    assert e_l <= b_l, f"loss |hip - fp64| = {e_l:.3e} > {b_l:.3e} (hip {lh.item():.9e}, fp64 {l64.item():.9e})"
    assert_fp64_truth(f"{name} alpha={alpha} d(sr)", gh, g32, g64)
    assert e_p <= b_p, f"pointwise gradient error {e_p:.3e} > {b_p:.3e}"


# ------------------------------------------------------------------------------------------------ B. closed forms on the device
# (H, W, u, v, the value in units of A^2): generic, DC, Nyquist on each axis and on both at 12 x 10; at 45 x 33 no Nyquist exists
COSINES = [(12, 10, 3, 2, 0.5), (12, 10, 0, 0, 1.0), (12, 10, 5, 0, 1.0), (12, 10, 0, 6, 1.0), (12, 10, 5, 6, 1.0), (12, 10, 5, 2, 0.5),
           (12, 10, 3, 6, 0.5), (45, 33, 7, 11, 0.5), (45, 33, 0, 0, 1.0), (45, 33, 16, 22, 0.5), (45, 33, 0, 9, 0.5), (45, 33, 16, 0, 0.5)]


@pytest.mark.parametrize("alpha", [0.0, 1.0, 2.0])
@pytest.mark.parametrize("H, W, u, v, value", COSINES)
def test_cosine_closed_form(H, W, u, v, value, alpha):
    A = 0.3
    _, gt = refs.images(31, 2, H, W)
    d = refs.cosine(A, u, v, H, W, torch.float32)
    got, expect = _loss(gt + d, gt, alpha), value * A * A
    print(f"[B cosine {H}x{W} ({u},{v}) alpha={alpha}] {got:.8e} expected {expect:.8e} rel {abs(got - expect) / expect:.2e}")
    assert abs(got - expect) <= CLOSED * expect


@pytest.mark.parametrize("alpha", [0.0, 1.0, 2.0])
@pytest.mark.parametrize("H, W", [(1, 1), (6, 1), (1, 7), (12, 10), (45, 33)])
def test_single_pixel_closed_form(H, W, alpha):
    a = 0.25
    gt = torch.zeros(2, 3, H, W)
    sr = gt.clone()
    sr[:, :, H // 2, W // 3] += a
    got, expect = _loss(sr, gt, alpha), a * a / (H * W)
    assert abs(got - expect) <= CLOSED * expect, (got, expect)


@pytest.mark.parametrize("name", ["even", "odd", "crop", "longest"])
def test_alpha_zero_is_the_library_mse(name):
    from srganst.loss import MSELoss
    x, gt = refs.case_images(name)
    got = _loss(x, gt, 0.0)
    mse = MSELoss()(x.cuda(), gt.cuda()).item()
    print(f"[B alpha=0 {name}] {got:.8e} MSELoss {mse:.8e} rel {abs(got - mse) / mse:.2e}")
    assert abs(got - mse) <= 1e-5 * mse


# ------------------------------------------------------------------------------------------------ C. structure
def test_batch_mean_transpose_and_roll():
    x, gt = refs.images(21, 3, 45, 70)
    x[1] = gt[1] + 0.5 * (x[1] - gt[1])                # make the images differ in more than their noise
    whole = _loss(x, gt)
    singles = [_loss(x[i:i + 1], gt[i:i + 1]) for i in range(3)]
    assert len(set(singles)) == 3
    assert abs(whole - sum(singles) / 3) <= 1e-6 * whole, (whole, singles)
    _, g = _hip(x, gt)
    lt, gT = _hip(x.transpose(2, 3).contiguous(), gt.transpose(2, 3).contiguous())
    assert abs(lt.item() - whole) <= CLOSED * whole, (lt.item(), whole)
    assert rel_err(gT.transpose(2, 3), g) <= CLOSED
    sh = (7, -11)
    lr_, gR = _hip(torch.roll(x, sh, (2, 3)), torch.roll(gt, sh, (2, 3)))
    assert abs(lr_.item() - whole) <= CLOSED * whole, (lr_.item(), whole)
    assert rel_err(gR, torch.roll(g, sh, (2, 3))) <= CLOSED      # the gradient rolls along with the inputs


def test_per_plane_normalisation():
    """Each plane is normalised by its own maximum: with only plane p differing the loss is that plane's contribution; the
    contributions add up; scaling d of one plane by c scales its contribution by c^2 and leaves the other planes' gradient bits."""
    x, gt = refs.images(22, 1, 40, 36)
    c, p = 3.0, 1
    d = x - gt
    d[0, 2] *= 0.1                                     # planes of different size: a shared maximum would show

    def only(q, scale=1.0):
        dd = torch.zeros_like(d)
        dd[0, q] = d[0, q] * scale
        return _loss(gt + dd, gt)
    parts = [only(q) for q in range(3)]
    whole = _loss(gt + d, gt)
    assert abs(whole - sum(parts)) <= CLOSED * whole, (whole, parts)
    assert abs(only(p, c) - c * c * parts[p]) <= CLOSED * c * c * parts[p]
    d2 = d.clone()
    d2[0, p] *= c
    assert abs(_loss(gt + d2, gt) - (whole + (c * c - 1) * parts[p])) <= CLOSED * (whole + (c * c - 1) * parts[p])
    _, g = _hip(gt + d, gt)
    _, g2 = _hip(gt + d2, gt)
    assert torch.equal(g2[0, 0], g[0, 0]) and torch.equal(g2[0, 2], g[0, 2])
    assert rel_err(g2[0, p], c * g[0, p]) <= CLOSED    # the weights do not change with the plane's scale: the gradient scales by c


@pytest.mark.parametrize("alpha", [0.0, 1.0, 2.0])
def test_identical_inputs_give_exact_zero(alpha):
    x, _ = refs.images(23, 2, 45, 33)
    l, g = _hip(x, x.clone(), alpha)
    assert l.item() == 0.0 and bool((g == 0).all())
    x2 = x.clone()
    x2[1, 2] += 0.05 * torch.randn(45, 33, generator=torch.Generator().manual_seed(1))
    l2, g2 = _hip(x2, x, alpha)                         # one differing plane among identical ones
    assert l2.item() > 0 and bool((g2[0] == 0).all()) and bool((g2[1, :2] == 0).all()) and bool(torch.isfinite(g2).all())


# ------------------------------------------------------------------------------------------------ D. protocol
@pytest.mark.parametrize("name", ["odd", "ragged"])
def test_scale_and_accumulate(name):
    x, gt = refs.case_images(name)
    xd, gd = x.cuda(), gt.cuda()
    loss, saved, scratch, counter = _raw(xd, gd)
    g0 = _raw_bwd(xd.shape, saved, scratch, torch.full_like(xd, float("nan")))
    torch.cuda.synchronize()
    assert counter.item() == 0                                          # the ticket counter re-armed itself
    assert bool(torch.isfinite(saved).all())                            # every element of the saved spectrum was written
    lh, gh = _hip(x, gt)
    assert loss.item() == lh.item() and rel_err(g0.cpu(), gh) <= 1e-6   # the module runs the same entries (gh went through * UP / UP)
    prefill = torch.randn(xd.shape, generator=torch.Generator().manual_seed(5)).cuda()
    acc = _raw_bwd(xd.shape, saved, scratch, prefill.clone(), accumulate=1)
    assert torch.equal(acc, prefill + g0)                               # scale 1: exactly the accumulate=0 gradient plus the prefill
    s_dev = torch.tensor(0.7, device="cuda")
    for kw, s in (({"scale_dev": s_dev}, 0.7), ({"scale_host": 0.25}, 0.25), ({"scale_dev": s_dev, "scale_host": 0.25}, 0.175)):
        gs = _raw_bwd(xd.shape, saved, scratch, torch.full_like(xd, float("nan")), **kw)
        assert rel_err(gs.cpu(), g0.cpu().double() * s) <= 1e-6, kw
        accs = _raw_bwd(xd.shape, saved, scratch, prefill.clone(), accumulate=1, **kw)
        assert torch.equal(accs, prefill + gs), kw


def test_two_eager_calls_give_equal_bits():
    term_checks.two_calls_give_equal_bits([lambda n=name: _hip(*refs.case_images(n)) for name in ("ragged", "crop")])


def test_graph_replay_matches_eager():
    from srganst.loss import FocalFrequencyLoss
    inputs = [refs.images(seed, 2, 48, 37) for seed in (501, 502, 503)]
    term_checks.graph_replay_matches_eager(FocalFrequencyLoss, inputs,
                                           lambda crit, xs: term_checks.ws_ptrs(crit, ("scratch", "partials", "counter")))


def test_no_grad_allocates_and_writes_no_spectrum(monkeypatch):
    from srganst.loss import FocalFrequencyLoss
    term_checks.no_grad_allocates_and_writes_nothing_saved(
        monkeypatch, FocalFrequencyLoss(), *refs.images(61, 2, 96, 96), saved_bytes=2 * 3 * 96 * 49 * 2 * 4, kernel="freq_weight_kernel",
        raw_loss=lambda xd, gd: _raw(xd, gd, want_saved=False)[0])


def test_nan_in_sr():
    x, gt = refs.images(71, 2, 48, 56)
    xb = x.clone()
    xb[0, 1, 30, 33] = float("nan")
    _, g = _hip(x, gt)
    lb, gb = _hip(xb, gt)                                               # the call returns
    assert bool(torch.isnan(lb))
    assert bool(torch.isnan(gb[0, 1]).all())                            # the transform is global: the whole plane
    assert bool(torch.isfinite(gb[1]).all()) and torch.equal(gb[1], g[1])
    assert torch.equal(gb[0, 0], g[0, 0]) and torch.equal(gb[0, 2], g[0, 2])


# ------------------------------------------------------------------------------------------------ E. in the engines
def _freq():
    from srganst.loss import FocalFrequencyLoss
    return FocalFrequencyLoss()


def test_warmup_engine_step_vs_oracle():
    term_checks.warmup_engine_step_vs_oracle(_freq, "Frequency", 1.0, refs.freq_loss)


def test_warmup_engine_graph_equals_eager():
    term_checks.warmup_engine_graph_equals_eager(_freq, "Frequency", 1.0)


def test_train_engine_graph_equals_eager():
    term_checks.train_engine_graph_equals_eager(_freq, "Frequency", 1.0)


# ------------------------------------------------------------------------------------------------ F. refusals
def test_refusals_launch_nothing(monkeypatch):
    x, gt = refs.images(81, 2, 24, 24)
    xd, gd = x.cuda(), gt.cuda()
    tall, wide = torch.zeros(1, 3, 513, 4, device="cuda"), torch.zeros(1, 3, 4, 513, device="cuda")
    crit = _freq()
    bad = {"cpu sr": (x, gd), "cpu gt": (xd, gt), "fp64": (xd.double(), gd.double()), "one channel": (xd[:, :1], gd[:, :1]),
           "shapes differ": (xd, gd[:1]), "H = 513": (tall, tall.clone(), "size 513x4 not built"),
           "W = 513": (wide, wide.clone(), "size 4x513 not built")}
    term_checks.refusals_launch_nothing(                                 # accepted: the smallest size, non-contiguous views
        monkeypatch, [(crit, *pair) for pair in bad.values()],
        [(crit, xd[:, :, :1, :1], gd[:, :, :1, :1]), (crit, xd[:, :, 3:20, 1:24:2], gd[:, :, 3:20, 1:24:2])], "freq_weight_kernel")
