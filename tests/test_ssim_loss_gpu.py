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
import torch.nn.functional as F

import ssim_refs as refs
from conftest import assert_fp64_truth, oracle_grads, rel_err

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
    for channel in ("y", "rgb"):
        x, gt, *_ = refs.case("ragged", channel)
        a, b = _hip(x, gt, channel), _hip(x, gt, channel)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("channel", ["y", "rgb"])
def test_graph_replay_matches_eager(channel):
    """Forward + backward captured after one warm-up call on a side stream (which allocates the criterion's workspace) and replayed
    on three inputs copied into the static tensors: loss and gradient bits equal the eager calls' each time, so the ticket counter
    re-arms inside the graph; no workspace is re-allocated."""
    from srganst.loss import SSIMLoss
    B, H, W = 2, 48, 40
    inputs = [refs.images(seed, B, H, W) for seed in (501, 502, 503)]

    def run(crit, xs, gs):
        loss = crit(xs, gs)
        (gx,) = torch.autograd.grad(loss, xs)
        return loss, gx

    eager = []
    for x, gt in inputs:
        loss, gx = run(SSIMLoss(channel), x.cuda().requires_grad_(True), gt.cuda())
        eager.append((loss.detach().clone(), gx.clone()))
    torch.cuda.synchronize()
    assert not torch.equal(eager[1][0], eager[2][0])

    crit = SSIMLoss(channel)
    xs = inputs[0][0].cuda().requires_grad_(True)
    gs = inputs[0][1].cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(crit, xs, gs)                                                # warm-up: allocates the workspace
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    ptrs = (crit._ws["partials"].data_ptr(), crit._ws["counter"].data_ptr())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, gx = run(crit, xs, gs)
    assert (crit._ws["partials"].data_ptr(), crit._ws["counter"].data_ptr()) == ptrs
    for k in (1, 2, 0):
        with torch.no_grad():
            xs.copy_(inputs[k][0])
            gs.copy_(inputs[k][1])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss, eager[k][0]), (k, loss, eager[k][0])
        assert torch.equal(gx, eager[k][1]), k
    del graph


# ------------------------------------------------------------------------------------------------ F. no_grad
@pytest.mark.parametrize("channel", ["y", "rgb"])
def test_no_grad_allocates_and_writes_no_maps(channel, monkeypatch):
    from srganst import ops
    from srganst.loss import SSIMLoss
    x, gt = refs.images(61, 2, 96, 96)
    xd, gd = x.cuda(), gt.cuda()
    map_bytes = 2 * (1 if channel == "y" else 3) * 86 * 86 * 3 * 4
    crit = SSIMLoss(channel)
    xg = xd.clone().requires_grad_(True)
    with_grad = crit(xg, gd)                                            # also allocates the workspace
    monkeypatch.setattr(ops, "TRACE_HBM", {})
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    with torch.no_grad():
        quiet = crit(xg, gd)
    plain = crit(xd, gd)                                                # grad mode on, sr does not require grad
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert torch.equal(quiet, with_grad) and torch.equal(plain, with_grad)
    assert not quiet.requires_grad and not plain.requires_grad
    calls = ops.TRACE_HBM["ssim_loss_fwd_kernel"]
    assert len(calls) == 2 and all(keep[3] is None for _, _, keep in calls)        # keep = (x, gt, loss, maps, ws)
    assert peak < map_bytes, (peak, map_bytes)                          # only the two 0-dim results were allocated
    # and through the ABI: a null maps pointer gives the same loss bits
    raw_loss, _, _ = _raw(xd, gd, 1 if channel == "y" else 3, want_maps=False)
    assert torch.equal(raw_loss, with_grad.detach())


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
def _reduced_cfg(rcb=2):
    from srganst.config import Config
    cfg = Config()
    cfg.MODEL.G_N_RCB = rcb
    return cfg


def test_warmup_engine_step_vs_oracle():
    """One eager warm-up step with Pixel (MSE) + 0.1 SSIM, B = 4, 96 -> 24 px, two residual blocks: SR, the logged values and every
    parameter gradient against the CPU oracle of mse + 0.1 * restatement (fp64-truth rule)."""
    from oracle import model as om
    from srganst.engine import WarmupEngine
    from srganst.loss import MSELoss, SSIMLoss
    from srganst.model import Generator
    cfg = _reduced_cfg()
    torch.manual_seed(41)
    G = Generator(cfg)
    sd0 = {k: v.clone() for k, v in G.state_dict().items()}
    gen = torch.Generator().manual_seed(42)
    gt = torch.rand(4, 3, 96, 96, generator=gen)
    lr = torch.rand(4, 3, 24, 24, generator=gen)

    def fl(sdx, lr_, gt_):
        sr_ = om.generator_forward(sdx, lr_, True, {})
        mse, ssim = F.mse_loss(sr_, gt_), refs.ssim_loss(sr_, gt_, "y")
        return mse + 0.1 * ssim, sr_, mse, ssim
    ins = ((lr, False), (gt, False))
    _, g32, _, (sr_ref, mse32, ssim32) = oracle_grads(fl, sd0, torch.float32, ins)
    _, g64, _, (_, mse64, ssim64) = oracle_grads(fl, sd0, torch.float64, ins)
    G.cuda().train()
    eng = WarmupEngine(cfg, G, {"Pixel": MSELoss(), "SSIM": SSIMLoss()}, {"Pixel": 1.0, "SSIM": 0.1}, use_graph=False)
    vals = eng.step(gt.cuda(), lr.cuda())
    assert rel_err(eng.sr.cpu(), sr_ref) < 1e-3
    assert list(vals) == ["Pixel", "SSIM"]
    assert abs(vals["Pixel"].item() - mse64.item()) <= 1e-3 * mse64.item()
    e = abs(vals["SSIM"].item() - 0.1 * ssim64.item())
    print(f"[H warm-up] SSIM term {vals['SSIM'].item():.7f} oracle fp64 {0.1 * ssim64.item():.7f} (fp32 {0.1 * ssim32.item():.7f})")
    assert e <= 1e-3 * 0.1 * ssim64.item()                              # SR itself carries 1e-3: the term is not held tighter
    report = []
    for n, p in G.named_parameters():
        assert_fp64_truth(n, p.grad.cpu(), g32[n], g64[n], report)
    print(f"[H warm-up] worst parameter-gradient error {max(r[1] for r in report):.3e}")
    eng.close()


def test_warmup_engine_graph_equals_eager():
    from srganst.engine import WarmupEngine
    from srganst.loss import MSELoss, SSIMLoss
    from srganst.model import Generator

    def run(use_graph):
        cfg = _reduced_cfg()
        torch.manual_seed(43)
        G = Generator(cfg).cuda().train()
        eng = WarmupEngine(cfg, G, {"Pixel": MSELoss(), "SSIM": SSIMLoss()}, {"Pixel": 1.0, "SSIM": 0.1}, use_graph=use_graph,
                           adam_capturable=True)
        gen = torch.Generator().manual_seed(44)
        logged = []
        for _ in range(3):
            gt = torch.rand(4, 3, 96, 96, generator=gen).cuda()
            lr = torch.rand(4, 3, 24, 24, generator=gen).cuda()
            logged.append({k: v.item() for k, v in eng.step(gt, lr).items()})
        torch.cuda.synchronize()
        assert eng.graph_active == use_graph
        sd = {k: v.clone() for k, v in G.state_dict().items()}
        eng.close()
        return sd, logged

    s1, l1 = run(False)
    s2, l2 = run(True)
    for k in s1:
        assert torch.equal(s1[k], s2[k]), k
    assert l1 == l2 and all(set(v) == {"Pixel", "SSIM"} for v in l1)


def test_train_engine_graph_equals_eager():
    """Adversarial + Pixel + SSIM in a reduced TrainEngine: the criterion sits in the two-branch graph beside the discriminator;
    replayed and eager steps leave the same bits (the pattern of tests/test_discriminator_gpu.py)."""
    from srganst.config import Config
    from srganst.engine import TrainEngine
    from srganst.loss import MSELoss, SSIMLoss
    from srganst.model import Discriminator, Generator

    def run(use_graph):
        cfg = Config()
        cfg.MODEL.G_N_CHANNEL, cfg.MODEL.G_N_RCB, cfg.MODEL.D_N_CHANNEL = 16, 2, 8
        torch.manual_seed(1)
        D, G = Discriminator(cfg).cuda().train(), Generator(cfg).cuda().train()
        cfg.add_g_criterion("Pixel", MSELoss(), 1.0)
        cfg.add_g_criterion("SSIM", SSIMLoss(), 0.1)
        cfg.SOLVER.D_UPDATE_INTERVAL = 1
        eng = TrainEngine(cfg, G, D, use_graph=use_graph, adam_capturable=True)
        gen = torch.Generator().manual_seed(2)
        for _ in range(4):
            gt = torch.rand(4, 3, 96, 96, generator=gen).cuda()
            lr = torch.rand(4, 3, 24, 24, generator=gen).cuda()
            eng.step(gt, lr)
        torch.cuda.synchronize()
        assert eng.graph_active == use_graph
        return G.state_dict(), D.state_dict(), {k: v.item() for k, v in eng.loss_values.items()}

    g1, d1, l1 = run(False)
    g2, d2, l2 = run(True)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    for k in d1:
        assert torch.equal(d1[k], d2[k]), k
    assert l1 == l2 and set(l1) == {"Adversarial", "Pixel", "SSIM"}


# ------------------------------------------------------------------------------------------------ I. refusals
def test_refusals_launch_nothing(monkeypatch):
    from srganst import ops
    from srganst._abi import HipPathError
    from srganst.loss import SSIMLoss
    x, gt = refs.images(81, 2, 24, 24)
    xd, gd = x.cuda(), gt.cuda()
    crit = SSIMLoss()
    monkeypatch.setattr(ops, "TRACE_HBM", {})
    bad = {"cpu sr": (x, gd), "cpu gt": (xd, gt), "fp64": (xd.double(), gd.double()), "one channel": (xd[:, :1], gd[:, :1]),
           "H = 10": (xd[:, :, :10], gd[:, :, :10]), "W = 10": (xd[:, :, :, :10], gd[:, :, :, :10]), "shapes differ": (xd, gd[:1])}
    for name, (a, b) in bad.items():
        with pytest.raises(HipPathError):
            crit(a, b)
    assert ops.TRACE_HBM == {} and crit._ws == {}
    assert torch.isfinite(crit(xd[:, :, :11, :11], gd[:, :, :11, :11]))    # the smallest accepted size, non-contiguous views
    assert list(ops.TRACE_HBM) == ["ssim_loss_fwd_kernel"]
