"""GPU: ArtifactLoss (csrc/artifact_loss.hip) held to the plain-torch restatement of its contract (tests/artifact_refs.py) under the
fp64-truth rule, and to its exact-zero, geometry, locality, scale / accumulate, determinism, graph capture, no_grad, NaN and refusal
rules; then inside WarmupEngine and TrainEngine, without and with the averaged generator as its reference.

fp64-truth rule (conftest): loss   |hip - l64| <= max(1e-3 |l64|, 3 |l32 - l64|)
                            grads  rel_err(hip, g64) <= max(1e-3, 3 rel_err(g32, g64)), and pointwise max|hip - g64| <= 1e-3 max|g64|
where l32 / g32 are the restatement in fp32 and l64 / g64 the same in fp64.

    tiny     1 x 4 x 4, k = 7      every tap is a reflection
    seams    2 x 33 x 65, k = 7    tile seams at 32 / 64, 1-px partial tiles, a ring that reflects inside a partial tile
    ragged   1 x 75 x 64, k = 7    three tile rows
    k3       2 x 19 x 43, k = 3    the smallest window
    k11      2 x 19 x 43, k = 11   the largest window
    medium   2 x 48 x 40, k = 7

Run with -s for the measured errors."""
import ctypes

import pytest
import torch

import artifact_refs as refs
import term_checks
from conftest import assert_fp64_truth, rel_err

pytestmark = pytest.mark.gpu

UP = 0.7                                              # non-unit upstream gradient


def _crit(ksize=7, refine=True):
    from srganst.loss import ArtifactLoss
    return ArtifactLoss(ksize, refine)


def _plain(ksize=7):
    return _crit(ksize, refine=False)


def _hip(x, gt, ref, ksize=7):
    """-> (loss, d loss / d sr) as fp64 host tensors; ref None: the unrefined criterion."""
    xg = x.cuda().requires_grad_(True)
    loss = _plain(ksize)(xg, gt.cuda()) if ref is None else _crit(ksize)(xg, gt.cuda(), ref.cuda())
    (gx,) = torch.autograd.grad(loss * UP, xg)
    torch.cuda.synchronize()
    return loss.detach().cpu().double(), gx.cpu().double() / UP


def _raw_fwd(x, gt, ref=None, ksize=7, want_map=True):
    """sst_artifact_loss_fwd straight through the C ABI on device tensors -> (loss, w map [B,H,W] or None, s_b [B] fp64, the two
    counters).  The map is NaN-prefilled."""
    from srganst import _abi
    B, _, H, W = x.shape
    nm, ns, npart = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    _abi.check(_abi.lib().sst_artifact_loss_workspace(B, H, W, ksize, ctypes.byref(nm), ctypes.byref(ns), ctypes.byref(npart)),
               "sst_artifact_loss_workspace")
    loss = torch.empty((), device="cuda")
    wmap = torch.full((nm.value,), float("nan"), device="cuda") if want_map else None
    stats = torch.empty(ns.value, device="cuda")
    partials = torch.empty(npart.value, device="cuda")
    counters = torch.zeros(2, device="cuda", dtype=torch.int32)
    _abi.check(_abi.lib().sst_artifact_loss_fwd(_abi.ptr(x), _abi.ptr(gt), _abi.ptr(ref), _abi.ptr(loss), _abi.ptr(wmap), _abi.ptr(stats),
                                                _abi.ptr(counters[0:1]), _abi.ptr(partials), _abi.ptr(counters[1:2]), B, H, W, ksize,
                                                _abi.stream_ptr()), "sst_artifact_loss_fwd")
    sb = stats.view(torch.float64)[-B:]
    return loss, None if wmap is None else wmap.view(B, H, W), sb, counters


def _raw_bwd(x, gt, wmap, dsr, scale_dev=None, scale_host=1.0, accumulate=0, ksize=7):
    from srganst import _abi
    B, _, H, W = x.shape
    _abi.check(_abi.lib().sst_artifact_loss_bwd(_abi.ptr(x), _abi.ptr(gt), _abi.ptr(wmap), _abi.ptr(dsr), _abi.ptr(scale_dev),
                                                float(scale_host), int(accumulate), B, H, W, ksize, _abi.stream_ptr()),
               "sst_artifact_loss_bwd")
    return dsr


# ------------------------------------------------------------------------------------------------ A. parity
@pytest.mark.parametrize("with_ref", [True, False], ids=["ref", "no ref"])
@pytest.mark.parametrize("name", list(refs.CASES))
def test_parity_vs_fp64(name, with_ref):
    x, gt, ref, l32, g32, l64, g64 = refs.case(name, with_ref)
    k = refs.CASES[name][4]
    lh, gh = _hip(x, gt, ref, k)
    e_l, b_l = abs(lh - l64).item(), max(1e-3 * abs(l64).item(), 3 * abs(l32 - l64).item())
    e_p, b_p = (gh - g64).abs().max().item(), 1e-3 * g64.abs().max().item()
    print(f"[A {name} {'ref' if with_ref else 'no ref'}] loss {lh.item():.7e} |hip-l64| {e_l:.3e} <= {b_l:.3e} | grad rel err "
          f"{rel_err(gh, g64):.3e} (fp32 restatement {rel_err(g32, g64):.3e}) | pointwise {e_p:.3e} <= {b_p:.3e}")
    assert torch.isfinite(lh) and bool(torch.isfinite(gh).all())
    assert e_l <= b_l, f"loss |hip - fp64| = {e_l:.3e} > {b_l:.3e} (hip {lh.item():.9e}, fp64 {l64.item():.9e})"
    assert_fp64_truth(f"{name} d(sr)", gh, g32, g64)
    assert e_p <= b_p, f"pointwise gradient error {e_p:.3e} > {b_p:.3e}"


@pytest.mark.parametrize("name", ["seams", "tiny"])
def test_saved_map_zero_set_is_the_fp64_mask(name):
    x, gt, ref, *_ = refs.case(name, True)
    k = refs.CASES[name][4]
    _, wmap, sb, _ = _raw_fwd(x.cuda(), gt.cuda(), ref.cuda(), k)
    want = refs.mask(x.double(), gt.double(), ref.double())[:, 0]
    assert torch.equal(wmap.cpu() == 0, want)
    w64 = refs.weight_map(x.double(), gt.double(), ref.double(), k)[:, 0]
    s64 = refs.global_weight(refs.residual(x.double(), gt.double()))
    print(f"[A {name}] w map rel err {rel_err(wmap.cpu().double(), w64):.3e}, s_b rel err {rel_err(sb.cpu(), s64):.3e}")
    assert rel_err(wmap.cpu().double(), w64) <= 1e-6 and rel_err(sb.cpu(), s64) <= 1e-12


# ------------------------------------------------------------------------------------------------ B. exact consequences
def test_identical_images_give_exactly_zero():
    x, _, ref = refs.images(91, 2, 33, 40)
    for k in (3, 7, 11):
        for r in (None, ref):
            l, g = _hip(x, x.clone(), r, k)
            assert l.item() == 0.0 and not bool(g.any()), (k, r is None)


def test_ref_is_sr_gives_the_bits_of_no_ref():
    x, gt, _ = refs.images(92, 2, 33, 40)
    xd, gd = x.cuda(), gt.cuda()
    xg = xd.clone().requires_grad_(True)
    la = _crit()(xg, gd, xg)
    (ga,) = torch.autograd.grad(la, xg)
    lb = _plain()(xg, gd)
    (gb,) = torch.autograd.grad(lb, xg)
    assert torch.equal(la, lb) and torch.equal(ga, gb) and la.item() > 0
    la_raw, wa, _, _ = _raw_fwd(xd, gd, xd)
    lb_raw, wb, _, _ = _raw_fwd(xd, gd, None)
    assert torch.equal(la_raw, lb_raw) and torch.equal(wa, wb) and torch.equal(la_raw, la.detach())


# ------------------------------------------------------------------------------------------------ C. geometry
def test_batch_mean_and_transpose():
    x, gt, ref = refs.images(21, 3, 45, 70)
    x[1] = gt[1] + 0.5 * (x[1] - gt[1])                # make the images differ in more than their noise
    xd, gd, rd = x.cuda(), gt.cuda(), ref.cuda()
    t = lambda a: a.transpose(2, 3).contiguous()
    for r in (None, ref):
        call = (lambda a, b, c: _plain()(a, b)) if r is None else (lambda a, b, c: _crit()(a, b, c))
        whole = call(xd, gd, rd).item()
        singles = [call(xd[i:i + 1], gd[i:i + 1], rd[i:i + 1]).item() for i in range(3)]
        assert len(set(singles)) == 3
        assert abs(whole - sum(singles) / 3) <= 1e-6 * abs(whole), (whole, singles)
        lt, g_t = _hip(t(x), t(gt), None if r is None else t(r))
        l, g = _hip(x, gt, r)
        assert abs(lt - l).item() <= 1e-6 * abs(l).item(), (lt, l)
        assert rel_err(g_t.transpose(2, 3), g) <= 1e-6


def test_locality():
    """A change of one sr value of image 0, next to a tile seam, that moves r there by 0.04: image 1's gradient keeps its bits;
    image 0's changes everywhere, through s_b; with s_b divided out of the saved maps only the k x k neighbourhood changes.  The maps
    are fp32: two roundings of 2^-24 each bound what w / s_b may differ by where the window did not change - asserted with 2^-22."""
    k, p = 7, 3
    x, gt, _ = refs.images(33, 2, 48, 56)
    qy, qx = 31, 33
    x2 = x.clone()
    x2[0, 1, qy, qx] += 0.04 * torch.sign(x[0, 1, qy, qx] - gt[0, 1, qy, qx])
    _, g = _hip(x, gt, None, k)
    _, g2 = _hip(x2, gt, None, k)
    assert torch.equal(g2[1], g[1])
    assert bool((g2[0] != g[0]).all())
    gd = gt.cuda()
    _, w, sb, _ = _raw_fwd(x.cuda(), gd, None, k)
    _, w2, sb2, _ = _raw_fwd(x2.cuda(), gd, None, k)
    assert torch.equal(w2[1], w[1]) and sb2[1].item() == sb[1].item() and sb2[0].item() != sb[0].item()
    u, u2 = (w[0].double() / sb[0]).cpu(), (w2[0].double() / sb2[0]).cpu()
    near = torch.zeros(48, 56, dtype=torch.bool)
    near[qy - p:qy + p + 1, qx - p:qx + p + 1] = True
    moved = (u2 - u).abs() > 2.0 ** -22 * u.abs()
    assert bool(moved[near].all()) and not bool(moved[~near].any())


# ------------------------------------------------------------------------------------------------ D. scale and accumulate
@pytest.mark.parametrize("name, with_ref", [("ragged", True), ("k11", False)])
def test_scale_and_accumulate(name, with_ref):
    x, gt, ref, *_ = refs.case(name, with_ref)
    k = refs.CASES[name][4]
    xd, gd, rd = x.cuda(), gt.cuda(), None if ref is None else ref.cuda()
    loss, wmap, _, counters = _raw_fwd(xd, gd, rd, k)
    bwd = lambda dsr, **kw: _raw_bwd(xd, gd, wmap, dsr, ksize=k, **kw)
    g0 = bwd(torch.full_like(xd, float("nan")))
    torch.cuda.synchronize()
    assert counters.tolist() == [0, 0]                                  # both ticket counters re-armed themselves
    assert bool(torch.isfinite(wmap).all()) and bool(torch.isfinite(g0).all())      # every element of the map and of d(sr) was written
    lh, gh = _hip(x, gt, ref, k)
    assert loss.item() == lh.item() and rel_err(g0.cpu(), gh) <= 1e-6   # the module runs the same entries (gh went through * UP / UP)
    prefill = torch.randn(xd.shape, generator=torch.Generator().manual_seed(5)).cuda()
    acc = bwd(prefill.clone(), accumulate=1)
    assert torch.equal(acc, prefill + g0)                               # scale 1: exactly the accumulate=0 gradient plus the prefill
    s_dev = torch.tensor(0.7, device="cuda")
    for kw, s in (({"scale_dev": s_dev}, 0.7), ({"scale_host": 0.25}, 0.25), ({"scale_dev": s_dev, "scale_host": 0.25}, 0.175)):
        gs = bwd(torch.full_like(xd, float("nan")), **kw)
        assert rel_err(gs.cpu(), g0.cpu().double() * s) <= 1e-6, kw
        accs = bwd(prefill.clone(), accumulate=1, **kw)
        assert torch.equal(accs, prefill + gs), kw


# ------------------------------------------------------------------------------------------------ E. determinism and capture
def test_two_eager_calls_give_equal_bits():
    x, gt, ref, *_ = refs.case("ragged", True)
    term_checks.two_calls_give_equal_bits([lambda: _hip(x, gt, ref), lambda: _hip(x, gt, None), lambda: _hip(x, gt, ref, 11)])


def _three_operand_run(crit, xs, gs):
    """gs holds gt and ref behind one another along the batch axis: the helper's two static tensors carry three operands."""
    B = xs.shape[0]
    loss = crit(xs, gs[:B], gs[B:])
    (gx,) = torch.autograd.grad(loss, xs)
    return loss, gx


@pytest.mark.parametrize("refine", [True, False], ids=["ref", "no ref"])
def test_graph_replay_matches_eager(refine):
    inputs = []
    for seed in (501, 502, 503):
        x, gt, ref = refs.images(seed, 2, 48, 40)
        inputs.append((x, torch.cat([gt, ref], 0)))
    keys = ("partials", "counter", "stat_partials", "stat_counter")
    term_checks.graph_replay_matches_eager(lambda: _crit(7, refine), inputs, lambda crit, xs: term_checks.ws_ptrs(crit, keys),
                                           run=_three_operand_run)


# ------------------------------------------------------------------------------------------------ F. no_grad
def test_no_grad_allocates_and_writes_no_map(monkeypatch):
    x, gt, _ = refs.images(61, 2, 96, 96)
    term_checks.no_grad_allocates_and_writes_nothing_saved(
        monkeypatch, _plain(), x, gt, saved_bytes=96 * 96 * 4, kernel="artifact_loss_fwd_kernel",
        raw_loss=lambda xd, gd: _raw_fwd(xd, gd, None, want_map=False)[0])


def test_no_grad_with_ref_allocates_and_writes_no_map(monkeypatch):
    """The same with the third operand: three images of algorithmic bytes, no map, nothing of a plane's size allocated."""
    from srganst import ops
    x, gt, ref = refs.images(61, 2, 96, 96)
    xd, gd, rd = x.cuda(), gt.cuda(), ref.cuda()
    crit = _crit()
    xg = xd.clone().requires_grad_(True)
    with_grad = crit(xg, gd, rd)
    monkeypatch.setattr(ops, "TRACE_HBM", {})
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    with torch.no_grad():
        quiet = crit(xg, gd, rd)
    plain = crit(xd, gd, rd)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert torch.equal(quiet, with_grad) and torch.equal(plain, with_grad) and not quiet.requires_grad and not plain.requires_grad
    calls = ops.TRACE_HBM["artifact_loss_fwd_kernel"]
    assert list(ops.TRACE_HBM) == ["artifact_loss_fwd_kernel"] and len(calls) == 2
    assert all(keep[3] is None and keep[5] is rd and nbytes == 3.0 * x.numel() * 4 for _, nbytes, keep in calls)
    assert peak < 96 * 96 * 4, peak
    assert torch.equal(_raw_fwd(xd, gd, rd, want_map=False)[0], with_grad.detach())


def test_gradient_for_gt_or_ref_is_refused():
    from srganst._abi import HipPathError
    x, gt, ref = (t.cuda() for t in refs.images(62, 1, 16, 16))
    with pytest.raises(HipPathError, match="with respect to sr only"):
        _plain()(x, gt.clone().requires_grad_(True)).backward()
    with pytest.raises(HipPathError, match="with respect to sr only"):
        _crit()(x, gt.clone().requires_grad_(True), ref).backward()
    with pytest.raises(HipPathError, match="with respect to sr only"):
        _crit()(x, gt, ref.clone().requires_grad_(True)).backward()


# ------------------------------------------------------------------------------------------------ G. NaN
def test_nan_in_sr():
    x, gt, ref = refs.images(71, 2, 48, 56)
    qy, qx = 30, 33
    xb = x.clone()
    xb[0, 1, qy, qx] = float("nan")
    gd = gt.cuda()
    _, g = _hip(x, gt, None)
    lb, gb = _hip(xb, gt, None)                                         # the call returns
    assert bool(torch.isnan(lb)) and bool(torch.isnan(gb[0]).all()) and torch.equal(gb[1], g[1])
    _, w, _, _ = _raw_fwd(x.cuda(), gd)
    lraw, wb, sbb, counters = _raw_fwd(xb.cuda(), gd)
    assert bool(torch.isnan(lraw)) and bool(torch.isnan(sbb[0])) and bool(torch.isnan(wb[0]).all())      # the whole map, through s_b
    assert torch.equal(wb[1], w[1]) and counters.tolist() == [0, 0]
    _, gr = _hip(x, gt, ref)
    lr_, gbr = _hip(xb, gt, ref)                                        # with ref: the masked pixels of image 0 stay 0
    assert bool(torch.isnan(lr_)) and torch.equal(gbr[1], gr[1]) and bool(torch.isnan(gbr[0, :, qy, qx]).all())


# ------------------------------------------------------------------------------------------------ H. refusals
class _WithRef:
    """crit(a, b, ref) as a criterion of two operands for term_checks.refusals_launch_nothing."""

    def __init__(self, crit, ref):
        self.crit, self.ref = crit, ref

    def __call__(self, a, b):
        return self.crit(a, b, self.ref)

    @property
    def _ws(self):
        return self.crit._ws


def test_refusals_launch_nothing(monkeypatch):
    x, gt, ref = refs.images(81, 2, 24, 24)
    xd, gd, rd = x.cuda(), gt.cuda(), ref.cuda()
    plain = _plain()
    bad = [(plain, x, gd), (plain, xd, gt), (plain, xd.double(), gd.double()), (plain, xd[:, :1], gd[:, :1]), (plain, xd, gd[:1]),
           (plain, xd[:, :, :3], gd[:, :, :3], "below the 4-px minimum"), (plain, xd[:, :, :, :3], gd[:, :, :, :3], "below the 4-px minimum"),
           (_plain(11), xd[:, :, :5], gd[:, :, :5], "below the 6-px minimum"),
           (_crit(), xd, gd, "SOLVER.G_EMA_DECAY"),                                           # refine=True without ref
           (_WithRef(_crit(), ref), xd, gd, "ref must be a tensor on a ROCm device"),
           (_WithRef(_crit(), rd.double()), xd, gd, "ref must be fp32"),
           (_WithRef(_crit(), rd[:1]), xd, gd, "ref must be fp32, of sr's shape"),
           (_WithRef(_crit(), rd[:, :, :20]), xd, gd, "of sr's shape"),
           (_WithRef(_crit(), rd), xd, gd[:, :, :20]),
           (_WithRef(_crit(), rd), xd[:, :, :20], gd)]
    ok = _WithRef(_crit(), rd[:, :, :4, :4])
    term_checks.refusals_launch_nothing(monkeypatch, bad, [(plain, xd[:, :, :4, :4], gd[:, :, :4, :4]), (ok, xd[:, :, :4, :4], gd[:, :, :4, :4])],
                                        "artifact_loss_fwd_kernel")
    for k in (2, 4, 12, 13, 1, 0, -7, 7.0, None):
        with pytest.raises(ValueError):
            _crit(k)


# ------------------------------------------------------------------------------------------------ I. in the engines, no reference
def test_warmup_engine_step_vs_oracle():
    term_checks.warmup_engine_step_vs_oracle(_plain, "Artifact", 1.0, lambda sr, gt: refs.artifact_loss(sr, gt))


def test_warmup_engine_graph_equals_eager():
    term_checks.warmup_engine_graph_equals_eager(_plain, "Artifact", 1.0)


def test_train_engine_graph_equals_eager():
    term_checks.train_engine_graph_equals_eager(_plain, "Artifact", 1.0)


# ------------------------------------------------------------------------------------------------ J. in the engines, refined
STEPS = 4


def _batches(seed):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.rand(4, 3, 96, 96, generator=gen).cuda(), torch.rand(4, 3, 24, 24, generator=gen).cuda()) for _ in range(STEPS)]


def _ema_on(cfg, decay=0.9):
    cfg.SOLVER.G_EMA_DECAY, cfg.SOLVER.G_EMA_WARMUP = decay, False
    return cfg


def _build(kind, use_graph, refine=True, decay=0.9, term=True):
    """The reduced configurations of term_checks with the averaged generator on -> (engine, G, D or None, config)."""
    from srganst.config import Config
    from srganst.engine import TrainEngine, WarmupEngine
    from srganst.loss import MSELoss
    from srganst.model import Discriminator, Generator
    if kind.startswith("warmup"):
        cfg = _ema_on(term_checks._reduced_cfg(), decay)
        torch.manual_seed(43)
        G = Generator(cfg).cuda().train()
        crits, weights = {"Pixel": MSELoss()}, {"Pixel": 1.0}
        if term:
            crits["Artifact"], weights["Artifact"] = _crit(7, refine), 1.0
        return WarmupEngine(cfg, G, crits, weights, use_graph=use_graph, adam_capturable=True, force_dp=kind == "warmup-dp"), G, None, cfg
    cfg = _ema_on(Config(), decay)
    cfg.MODEL.G_N_CHANNEL, cfg.MODEL.G_N_RCB, cfg.MODEL.D_N_CHANNEL = 16, 2, 8
    cfg.KERNEL.OVERLAP_GD = kind == "train"              # "train": the whole iteration as one graph; "train-split": a graph per half
    torch.manual_seed(1)
    D, G = Discriminator(cfg).cuda().train(), Generator(cfg).cuda().train()
    cfg.add_g_criterion("Pixel", MSELoss(), 1.0)
    if term:
        cfg.add_g_criterion("Artifact", _crit(7, refine), 1.0)
    cfg.SOLVER.D_UPDATE_INTERVAL = 1
    return TrainEngine(cfg, G, D, use_graph=use_graph, adam_capturable=True, force_dp=kind == "train-dp"), G, D, cfg


def _logged(eng):
    return {k: v.item() for k, v in eng.loss_values.items()}


def _run(kind, use_graph):
    eng, G, D, _ = _build(kind, use_graph)
    logged, refs_seen = [], []
    for gt, lr in _batches(44):
        eng.step(gt, lr)
        logged.append(_logged(eng))
        refs_seen.append(eng.sr_ref.clone())
    torch.cuda.synchronize()
    assert eng.graph_active == use_graph
    out = {"G." + k: v.clone() for k, v in G.state_dict().items()}
    out.update({"ema." + k: v.clone() for k, v in eng.g_ema.state_dict().items()})
    if D is not None:
        out.update({"D." + k: v.clone() for k, v in D.state_dict().items()})
    eng.close()
    return out, logged, refs_seen


@pytest.mark.parametrize("kind", ["warmup", "warmup-dp", "train", "train-split", "train-dp"])
def test_refined_engine_graph_equals_eager(kind):
    """4 steps with ArtifactLoss(refine=True), G_EMA_DECAY = 0.9, G_EMA_WARMUP off: replayed and eager steps leave the same bits in
    G, D, the averaged generator (weights and the copied BatchNorm buffers), the logged values and the reference image."""
    s1, l1, r1 = _run(kind, False)
    s2, l2, r2 = _run(kind, True)
    assert set(s1) == set(s2)
    for k in s1:
        assert torch.equal(s1[k], s2[k]), k
    assert l1 == l2 and all("Artifact" in v and v["Artifact"] > 0 for v in l1)
    assert all(torch.equal(a, b) for a, b in zip(r1, r2))
    assert not torch.equal(r1[2], r1[3])


@pytest.mark.parametrize("kind", ["warmup", "train"])
def test_reference_follows_the_step_order_rule(kind):
    """ref at step t is the eval-mode forward with the averaged weights and G's running statistics as step t-1 left them: at steps
    0, 1 and 3, eng.sr_ref equals the forward of a fresh generator loaded with exactly those; the logged term is the criterion of
    (eng.sr, gt, eng.sr_ref) times its weight, bit for bit.  At step 0 the averaged weights are G's, but ref is an eval-mode forward
    (running statistics 0 / 1) while sr is a training-mode one (batch statistics), so ref differs from sr and the mask is not empty
    there: the term is held to the refined value of (eng.sr, gt, eng.sr_ref), and shown to lie strictly below the unrefined one.
    Measured on an MI355X at step 0: masked share 0.497 (warm-up) / 0.512 (train), logged 4.976e-2 / 4.960e-2 against an unrefined
    8.483e-2 / 8.581e-2 - an equality of the logged term with the unrefined value cannot hold for an eval-mode reference."""
    from srganst.model import Generator
    eng, G, _, cfg = _build(kind, False)
    fresh = Generator(cfg).cuda().eval()
    for t, (gt, lr) in enumerate(_batches(44)):
        weights = {k: v.clone() for k, v in eng.g_ema.named_parameters()}
        stats = {k: v.clone() for k, v in G.named_buffers()}
        if t == 0:
            assert all(torch.equal(weights[k], p) for k, p in G.named_parameters())      # the average starts as G
        eng.step(gt, lr)
        if t not in (0, 1, 3):
            continue
        fresh.load_state_dict({**weights, **stats})
        with torch.no_grad():
            want = fresh(lr)
        assert torch.equal(eng.sr_ref, want), t
        assert not eng.sr_ref.requires_grad and not torch.equal(eng.sr_ref, eng.sr)
        with torch.no_grad():
            refined, plain = _crit()(eng.sr, gt, eng.sr_ref), _plain()(eng.sr, gt)
        logged = eng.loss_values["Artifact"]
        share = float((refs.residual(eng.sr, gt) < refs.residual(eng.sr_ref, gt)).float().mean())
        print(f"[J {kind} step {t}] logged {logged.item():.7e} refined {refined.item():.7e} unrefined {plain.item():.7e} masked share {share:.3f}")
        assert torch.equal(logged, refined) and refined.item() < plain.item()
    eng.close()


def test_engines_refuse_the_refined_term_without_an_average():
    for kind in ("warmup", "train"):
        with pytest.raises(ValueError, match="G_EMA_DECAY"):
            _build(kind, False, decay=0.0)
        eng, *_ = _build(kind, False, refine=False, decay=0.0)           # the unrefined term needs none
        assert eng.g_ema is None and eng.sr_ref is None
        eng.close()


def _trace_of_a_step(monkeypatch, kind, **kw):
    """-> ({kernel name: launches} of one eager step over both launch seams, torch._foreach_copy_ calls, eng.sr_ref)."""
    from srganst import ops
    eng, *_ = _build(kind, False, **kw)
    gt, lr = _batches(44)[0]
    eng.step(gt, lr)                                                    # allocates workspaces
    copies = []
    real = torch._foreach_copy_
    monkeypatch.setattr(torch, "_foreach_copy_", lambda *a, **k: (copies.append(len(a[0])), real(*a, **k))[1])
    monkeypatch.setattr(ops, "TRACE", {})
    monkeypatch.setattr(ops, "TRACE_HBM", {})
    eng.step(gt, lr)
    torch.cuda.synchronize()
    counts = {k: len(v) for k, v in {**ops.TRACE, **ops.TRACE_HBM}.items()}
    monkeypatch.setattr(ops, "TRACE", None)
    monkeypatch.setattr(ops, "TRACE_HBM", None)
    monkeypatch.setattr(torch, "_foreach_copy_", real)
    sr_ref = eng.sr_ref
    eng.close()
    return counts, copies, sr_ref


@pytest.mark.parametrize("kind", ["warmup", "train"])
def test_a_step_without_the_term_launches_what_it_launched(monkeypatch, kind):
    """With the average on: a step without the term, and one with the unrefined term, launch neither the buffer copy nor a second
    generator forward - the unrefined term adds exactly its own forward and backward entry; the refined term adds one multi-tensor
    copy call and the convolutions of one more forward."""
    ours = {"artifact_loss_fwd_kernel": 1, "artifact_loss_bwd_kernel": 1}
    base, copies0, ref0 = _trace_of_a_step(monkeypatch, kind, term=False)
    plain, copies1, ref1 = _trace_of_a_step(monkeypatch, kind, refine=False)
    refined, copies2, ref2 = _trace_of_a_step(monkeypatch, kind, refine=True)
    assert not any(k.startswith("artifact") for k in base) and copies0 == [] and ref0 is None
    assert plain == {**base, **ours} and copies1 == [] and ref1 is None
    assert copies2 and len(copies2) == 1 and ref2 is not None
    assert {k: refined[k] for k in ours} == ours and set(refined) >= set(plain)
    more = {k: refined[k] - plain.get(k, 0) for k in refined if refined[k] != plain.get(k, 0)}
    print(f"[J {kind}] the reference forward adds {more}")
    assert more and all(v > 0 for v in more.values())
