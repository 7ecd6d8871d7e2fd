"""GPU: the small layout / criterion kernels of csrc/misc.hip held to plain torch on the CPU (fp64 where arithmetic is involved):
NCHW<->NHWC hand-offs, clamp backward with its fp64 bias column sum, the pixel / feature / BCE criteria, the VGG pool, the loss
sum and the un-rounded bicubic.

Rules (tests/glue_refs.py holds the formulas, tests/test_glue_references.py holds those to autograd on the CPU):
  data movement / selection            bitwise (value-equal where only the sign of a zero could differ; NaN positions equal)
  elementwise fp32 chains              |hip - ref64| <= k * 2^-24 * sum|terms| per element, k = fp32 roundings, written at each use
  reductions                           conftest.assert_fp64_truth: rel err <= max(1e-3, 3 x rel err of the same formula in fp32 torch)
Outputs live between sentinel-filled guard bands.  Run with -s for the error tables."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import glue_refs as G
from conftest import assert_fp64_truth

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from srganst import ops
    return ops


def dev(t):
    return None if t is None else t.detach().to(torch.float32).contiguous().cuda()


def same_values(a, b):
    """Equal as numbers, NaN in the same places."""
    a, b = a.cpu(), b.cpu()
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


# ================================================================================================ transposes
SHAPES = [(1, 1, 1, 1), (2, 3, 5, 7), (3, 64, 13, 9), (2, 3, 300, 301)]       # the last: more than 1024 * 256 elements (grid stride)


@pytest.mark.parametrize("B, C, H, W", SHAPES)
def test_transpose_both_directions(ops, B, C, H, W):
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(B * C * H))
    with G.Guarded().patch(ops):
        nhwc = ops.transpose(dev(x), to_nchw=False)
        back = ops.transpose(nhwc, to_nchw=True)
    assert torch.equal(nhwc.cpu(), x.permute(0, 2, 3, 1).contiguous())
    assert torch.equal(back.cpu(), x)


@pytest.mark.parametrize("with_shift", [True, False])
@pytest.mark.parametrize("B, C, H, W", SHAPES)
def test_transpose_affine(ops, B, C, H, W, with_shift):
    """v*scale[c] + shift[c] in one fmaf: k = 1."""
    gen = torch.Generator().manual_seed(B * C * H + with_shift)
    x = torch.randn(B, C, H, W, generator=gen)
    sc = torch.randn(C, generator=gen)
    sh = torch.randn(C, generator=gen) if with_shift else None
    with G.Guarded().patch(ops):
        nhwc = ops.transpose_affine(dev(x), False, dev(sc), dev(sh))
        nchw = ops.transpose_affine(dev(x.permute(0, 2, 3, 1)), True, dev(sc), dev(sh))
    prod = x.double() * sc.double().view(1, -1, 1, 1)
    ref = prod + (sh.double().view(1, -1, 1, 1) if with_shift else 0.0)
    terms = prod.abs() + (sh.double().abs().view(1, -1, 1, 1) if with_shift else 0.0)
    G.assert_elementwise("transpose_affine to NHWC", nhwc, ref.permute(0, 2, 3, 1), terms.permute(0, 2, 3, 1), 1)
    G.assert_elementwise("transpose_affine to NCHW", nchw, ref, terms, 1)


# ================================================================================================ clamp backward
EDGES = [-0.0, 0.0, 1.0, float(np.nextafter(np.float32(1), np.float32(2))), float(np.nextafter(np.float32(0), np.float32(-1))), NAN]


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("B, H, W", [(16, 96, 96), (2, 17, 23), (3, 300, 301)])
def test_clamp_bwd(ops, B, C, H, W):
    """The mask (0 <= pre <= 1, NaN outside) equals torch's clamp backward on the same input; dbias is the column sum of the masked
    gradient (fp64 rule), written and accumulated.  (3, 300, 301): more pixels than 1024 * 256, the grid-stride loop."""
    report = []
    gen = torch.Generator().manual_seed(B * H + C)
    pre = torch.rand(B, C, H, W, generator=gen) * 1.6 - 0.3
    g = torch.randn(B, C, H, W, generator=gen)
    flat = pre.view(-1)
    pos = [0, 1, 2, 3, 4, 5, flat.numel() - 1, flat.numel() // 2] + torch.randint(0, flat.numel(), (64,), generator=gen).tolist()
    for i, p in enumerate(pos):
        flat[p] = EDGES[i % len(EDGES)]
    leaf = pre.clone().requires_grad_(True)
    leaf.clamp(0, 1).backward(g)
    ref = leaf.grad.permute(0, 2, 3, 1).contiguous()
    assert torch.equal(leaf.grad != 0, G.clamp_mask(pre))
    col64, col32 = ref.double().sum((0, 1, 2)), ref.sum((0, 1, 2))
    pre_b = torch.randn(C, generator=gen)
    gd = G.Guarded()
    with gd.patch(ops):
        db, db_acc = gd.empty(C), gd.put(pre_b)
        out = ops.clamp_bwd(dev(g), dev(pre), db)
        out2 = ops.clamp_bwd(dev(g), dev(pre), db_acc, accumulate=True)
        out3 = ops.clamp_bwd(dev(g), dev(pre))
    for o in (out, out2, out3):
        assert torch.equal(o.cpu(), ref), "clamp mask differs from torch's clamp backward"
    assert_fp64_truth(f"dbias C={C} {B, H, W}", db.cpu(), col32.double(), col64, report)
    assert_fp64_truth(f"dbias+= C={C} {B, H, W}", db_acc.cpu(), (col32 + pre_b).double(), col64 + pre_b.double(), report)
    G.print_report(f"clamp_bwd C={C} {B, H, W}", report)


# ================================================================================================ pixel criterion
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [1, 3, 5, 1023, 1024, 1025, 8 * 3 * 192 * 192 + 2])
def test_pixel_loss(ops, n, mode):
    """Loss: fp64 rule; the n % 4 tail belongs to block 0.  Gradient, elementwise: k = 5 on |g| + |prefill| (a - b, scale/n, * scale_dev,
    * 2d, the accumulate); the counter is left zero and a second launch is bit-identical."""
    report = []
    gen = torch.Generator().manual_seed(n + mode)
    x, gt = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    gt[::7] = x[::7]                                              # d == 0 exactly
    x[n // 2] = 0.0
    sdev, shost = torch.tensor([0.7]), 1.5
    pre = torch.randn(n, generator=gen)
    gd = G.Guarded()
    ws = {}
    with gd.patch(ops):
        l1 = ops.pixel_loss_fwd(dev(x), dev(gt), mode, ws)
        assert int(ws["counter"].item()) == 0, "the last-block counter must be left zero"
        l2 = ops.pixel_loss_fwd(dev(x), dev(gt), mode, ws)
        assert int(ws["counter"].item()) == 0
        g_plain = ops.pixel_loss_bwd(dev(x), dev(gt), mode)
        g_acc = ops.pixel_loss_bwd(dev(x), dev(gt), mode, scale_dev=dev(sdev), scale_host=shost, out=gd.put(pre), accumulate=True)
    assert torch.equal(l1.cpu(), l2.cpu())
    G.assert_scalar_truth(f"pixel_loss n={n} mode={mode}", l1, G.pixel_loss(x, gt, mode), G.pixel_loss(x.double(), gt.double(), mode),
                          report)
    g64 = G.pixel_loss_grad(x.double(), gt.double(), mode)
    G.assert_elementwise("pixel_loss_bwd", g_plain, g64, g64.abs(), 5)
    s = float(sdev.double()) * shost
    G.assert_elementwise("pixel_loss_bwd scaled, accumulated", g_acc, pre.double() + s * g64, pre.double().abs() + (s * g64).abs(), 5)
    G.print_report(f"pixel_loss n={n} mode={mode}", report)


# ================================================================================================ feature criterion
def _feat_abi(x, gt, scale, shift, slope, C, mode, gd, dx=None, scale_dev=None, scale_host=1.0, accumulate=0):
    from srganst import _abi
    from srganst._abi import check, ptr, stream_ptr
    L, n = _abi.lib(), x.numel()
    if dx is None:
        loss, partials = gd.empty(()), gd.empty(L.sst_pixel_loss_blocks(n))
        counter = gd.empty(1, dtype=torch.int32, fill=0)
        check(L.sst_feat_loss_fwd(ptr(x), ptr(gt), ptr(scale), ptr(shift), slope, C, ptr(loss), ptr(partials), ptr(counter), n, mode,
                                  stream_ptr()), "sst_feat_loss_fwd")
        return loss, counter
    check(L.sst_feat_loss_bwd(ptr(x), ptr(gt), ptr(scale), ptr(shift), slope, C, ptr(dx), ptr(scale_dev), scale_host, accumulate, n, mode,
                              stream_ptr()), "sst_feat_loss_bwd")
    return dx


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("slope", [0.0, 0.2])
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("C, rows", [(1, 1), (1, 777), (64, 300), (96, 4099)])
def test_feat_loss(C, rows, affine, slope, mode):
    """crit(lrelu(x*s + t) - lrelu(gt*s + t)), mode 0 = MSE / 1 = L1, against the formula's fp64 autograd (test_glue_references) -
    loss under the fp64 rule; gradient elementwise with T = |x s| + |gt s| + 2|t| (the terms of d = a - b):
      MSE  k = 8 on 2 T |act' s| / n : two fmaf, two slope products, a - b, scale/n, * scale_dev, * 2d, * (act' s) (2)  - rounded up;
      L1   the gradient is +-(act' s)/n, k = 4; where |d| is within 4 roundings of T the fp32 sign of d may be 0 or the other sign's
           neighbour, there the magnitude alone is held."""
    report = []
    gen = torch.Generator().manual_seed(C * rows + mode)
    x, gt = torch.randn(rows, C, generator=gen), torch.randn(rows, C, generator=gen)
    gt.view(-1)[::5] = x.view(-1)[::5]                            # x == gt
    sc, sh = (torch.randn(C, generator=gen), torch.randn(C, generator=gen)) if affine else (None, None)
    slope32 = float(np.float32(slope))
    sdev, shost = torch.tensor([0.7]), 1.5
    pre = torch.randn(rows, C, generator=gen)
    gd = G.Guarded()
    xd, gtd, scd, shd = dev(x), dev(gt), dev(sc), dev(sh)
    l1, counter = _feat_abi(xd, gtd, scd, shd, slope, C, mode, gd)
    l2, _ = _feat_abi(xd, gtd, scd, shd, slope, C, mode, gd)
    g_plain = _feat_abi(xd, gtd, scd, shd, slope, C, mode, gd, dx=gd.empty(rows, C))
    g_acc = _feat_abi(xd, gtd, scd, shd, slope, C, mode, gd, dx=gd.put(pre), scale_dev=dev(sdev), scale_host=shost, accumulate=1)
    gd.check()
    assert int(counter.item()) == 0 and torch.equal(l1.cpu(), l2.cpu())
    d = lambda t: None if t is None else t.double()
    G.assert_scalar_truth(f"feat_loss C={C} rows={rows} affine={affine} slope={slope} mode={mode}", l1,
                          G.feat_loss(x, gt, sc, sh, slope32, mode), G.feat_loss(d(x), d(gt), d(sc), d(sh), slope32, mode), report)
    g64 = G.feat_loss_grad(d(x), d(gt), d(sc), d(sh), slope32, mode)
    s1 = d(sc).abs() if affine else torch.ones(C, dtype=torch.float64)
    T = (d(x).abs() + d(gt).abs()) * s1 + (2 * d(sh).abs() if affine else 0.0)
    za = G.feat_act(d(x), d(sc), d(sh), slope32)[0]
    unit = torch.where(za > 0, torch.ones_like(za), torch.full_like(za, slope32)) * s1 / x.numel()      # |d g / d (sign or 2d)|
    s = float(sdev.double()) * shost
    if mode == 0:
        G.assert_elementwise("feat_loss_bwd MSE", g_plain, g64, 2 * T * unit, 8)
        G.assert_elementwise("feat_loss_bwd MSE scaled, accumulated", g_acc, d(pre) + s * g64, d(pre).abs() + s * 2 * T * unit, 8)
    else:
        dd = G.feat_act(d(x), d(sc), d(sh), slope32)[1] - G.feat_act(d(gt), d(sc), d(sh), slope32)[1]
        near = dd.abs() <= 4 * G.U24 * T
        hp, ha = g_plain.cpu().double(), g_acc.cpu().double() - d(pre)
        assert bool(((hp - g64).abs() <= 4 * G.U24 * unit)[~near].all())
        assert bool((hp.abs() <= unit * (1 + 4 * G.U24))[near].all())
        assert bool(((ha - s * g64).abs() <= 6 * G.U24 * (d(pre).abs() + s * unit))[~near].all())
        assert bool((hp[gt == x] == 0).all())
    G.print_report(f"feat_loss C={C} rows={rows}", report)


# ================================================================================================ BCE with logits
SPECIAL = [100.0, -100.0, 20.0, -20.0, 0.0]


def _bce_check(ops, x, target, report, tag):
    """Loss: fp64 rule.  dlogits = scale (sigmoid(x) - t) / n, elementwise on |sigmoid| + |t|: k = 8 (expf within 2 ulp, 1 + e, the
    reciprocal, - t, scale/n, * scale_dev, the product)."""
    t32 = float(np.float32(target))
    n = x.numel()
    sdev, shost = torch.tensor([0.7]), 1.5
    gd = G.Guarded()
    with gd.patch(ops):
        l_only, none = ops.bce_logits(dev(x), target, want_loss=True, want_grad=False)
        none2, g_only = ops.bce_logits(dev(x), target, want_loss=False, want_grad=True)
        l_both, g_both = ops.bce_logits(dev(x), target, want_loss=True, want_grad=True, scale_dev=dev(sdev), scale_host=shost)
    assert none is None and none2 is None
    assert same_values(l_only, l_both)
    finite = ~torch.isnan(x)
    if bool(finite.all()):
        tt = torch.full_like(x, t32)
        l64 = F.binary_cross_entropy_with_logits(x.double(), tt.double())
        assert float((l64 - G.bce_loss(x.double(), t32)).abs()) <= 1e-12 * max(1.0, float(l64))
        G.assert_scalar_truth(f"bce {tag}", l_only, F.binary_cross_entropy_with_logits(x, tt), l64, report)
    else:
        assert math.isnan(l_only.item()), "a NaN logit must give a NaN loss"
    g64 = G.bce_grad(x.double(), t32)
    terms = (torch.sigmoid(x.double()) + abs(t32)) / n
    s = float(sdev.double()) * shost
    for name, h, k in (("grad only", g_only, 1.0), ("loss + grad, scaled", g_both, s)):
        h = h.cpu()
        assert torch.equal(torch.isnan(h), ~finite), f"bce {tag} {name}: NaN positions"
        G.assert_elementwise(f"bce dlogits {tag} {name}", h[finite], k * g64[finite], k * terms[finite], 8)


@pytest.mark.parametrize("target", [0.0, 1.0, 0.9])
@pytest.mark.parametrize("n", [1, 16, 257])
def test_bce_logits(ops, n, target):
    report = []
    gen = torch.Generator().manual_seed(n)
    if n == 1:
        cases = [torch.tensor([v]) for v in SPECIAL + [NAN, 0.37]]
    else:
        x = 3 * torch.randn(n, generator=gen)
        x[:len(SPECIAL)] = torch.tensor(SPECIAL)
        x[-1] = -100.0
        xn = x.clone()
        xn[n // 2] = NAN
        cases = [x, xn]
    for i, x in enumerate(cases):
        _bce_check(ops, x.view(-1, 1), target, report, f"n={n} t={target} case {i}")
    G.print_report(f"bce_logits n={n} t={target}", report)


# ================================================================================================ VGG pool
def _pool_input(B, C, H, W, seed):
    """NCHW input whose first windows are: all negative, all zero, mixed -0.0 / 0.0, exact ties (all four, two positive and equal, a
    tie with the maximum last), one NaN in each of the four positions (others positive / others negative)."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=gen)
    wins = [[-1.0, -2.0, -0.5, -3.0], [0.0] * 4, [-0.0, 0.0, -0.0, 0.0], [2.0] * 4, [1.5, -1.0, 1.5, 0.5], [0.25, 0.75, 0.5, 0.75]]
    for p in range(4):
        for base in ([0.5, 1.0, 2.0, 3.0], [-0.5, -1.0, -2.0, -3.0]):
            w = list(base)
            w[p] = NAN
            wins.append(w)
    wo = W // 2
    slots = (H // 2) * wo
    for c in range(C):
        for i, w in enumerate(wins):
            s = (i + 3 * c) % slots if slots >= len(wins) else i
            if s >= slots:
                continue
            oy, ox = divmod(s, wo)
            x[c % B, c, 2 * oy:2 * oy + 2, 2 * ox:2 * ox + 2] = torch.tensor(w).view(2, 2)
    return x


@pytest.mark.parametrize("B, C, H, W", [(2, 4, 8, 10), (1, 64, 8, 8), (2, 512, 6, 6), (3, 64, 150, 152), (1, 4, 2, 2)])
def test_maxpool_relu(ops, B, C, H, W):
    """Forward against F.max_pool2d(F.relu(x), 2), backward against its autograd on the same input, value for value: ties go to the
    first maximum, a NaN in a window comes out as NaN and takes the gradient.  (3, 64, 150, 152): beyond the 1024-workgroup stride."""
    x = _pool_input(B, C, H, W, B * C + H)
    if B * (H // 2) * (W // 2) * (C // 4) > 1024 * 256:
        assert G.grid_for(B * (H // 2) * (W // 2) * (C // 4), 1024) == 1024
    up = torch.randn(B, C, H // 2, W // 2, generator=torch.Generator().manual_seed(5))
    leaf = x.clone().requires_grad_(True)
    ref = F.max_pool2d(F.relu(leaf), 2)
    ref.backward(up)
    if H * W >= 64:
        assert int(torch.isnan(ref).sum()) >= 8
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    with G.Guarded().patch(ops):
        out = ops.maxpool_relu_fwd(dev(nhwc(x)))
        dy = ops.maxpool_relu_bwd(dev(nhwc(up)), dev(nhwc(x)))
    assert same_values(out, nhwc(ref.detach())), "forward differs from F.max_pool2d(F.relu(x), 2) (NaN must come through)"
    assert same_values(dy, nhwc(leaf.grad)), "backward sends a gradient elsewhere than torch"


# ================================================================================================ loss sum
@pytest.mark.parametrize("with_weighted", [True, False])
@pytest.mark.parametrize("n", range(0, 10))
def test_weighted_sum(n, with_weighted):
    """weighted[i] = w[i] * term[i]: one product, bit-equal to torch's fp32 product.  out = their sum in order: k = n roundings (the
    adds; a product fused into its add only removes one) on sum |w term|.  n = 0 and n = 9 are rejected before any launch."""
    from srganst import _abi
    from srganst._abi import HipPathError, check, ptr, stream_ptr
    gen = torch.Generator().manual_seed(n)
    m = max(n, 1)
    terms, w = torch.randn(m, generator=gen), torch.randn(m, generator=gen)
    gd = G.Guarded()
    tds = [dev(terms[i].reshape(())) for i in range(m)]
    out = gd.empty((), fill=G.SENTINEL)
    weighted = gd.empty(m, fill=G.SENTINEL) if with_weighted else None
    ptrs = (ctypes.c_void_p * m)(*[ptr(t) for t in tds])
    wts = (ctypes.c_float * m)(*[float(v) for v in w])
    rc = _abi.lib().sst_weighted_sum(ptrs, wts, n, ptr(out), ptr(weighted), stream_ptr())
    gd.check()
    if n in (0, 9):
        with pytest.raises(HipPathError):
            check(rc, "sst_weighted_sum")
        assert out.item() == pytest.approx(G.SENTINEL)
        return
    check(rc, "sst_weighted_sum")
    if with_weighted:
        assert torch.equal(weighted.cpu(), terms * w)
    prod = terms.double() * w.double()
    G.assert_elementwise("weighted_sum", out.reshape(1), prod.sum().reshape(1), prod.abs().sum().reshape(1), n + 1)


# ================================================================================================ bicubic without the 1/255 grid
@pytest.mark.parametrize("planes, H, W, scale", [(6, 40, 28, 0.25), (3, 24, 36, 0.25), (2, 17, 12, 0.5), (1, 8, 20, 2.0)])
def test_bicubic_unrounded(planes, H, W, scale):
    """round_grid = 0, non-square, against the host path of srganst/bicubic.py in fp64 with the same fp32 tap tables: per output
    pixel k = Ty + Tx + 2 roundings (a product and an add per tap, fused or not) on sum_tx |wx| sum_ty |wy x|."""
    from srganst import _abi
    from srganst._abi import check, ptr, stream_ptr
    from srganst.bicubic import Bicubic
    bic = Bicubic("cpu")
    wy, iy, wx, ix = bic.tables(H, W, scale, "cpu")
    oh, ow = int(H * scale), int(W * scale)
    assert oh != ow and tuple(wy.shape) == tuple(iy.shape) and wy.shape[0] == oh and wx.shape[0] == ow
    x = torch.rand(planes, H, W, generator=torch.Generator().manual_seed(H * W))
    gd = G.Guarded()
    y = gd.empty(planes, oh, ow)
    xd, wyd, wxd = dev(x), dev(wy), dev(wx)
    iyd, ixd = iy.to(torch.int32).contiguous().cuda(), ix.to(torch.int32).contiguous().cuda()
    check(_abi.lib().sst_bicubic(ptr(xd), ptr(y), ptr(wyd), ptr(iyd), ptr(wxd), ptr(ixd), planes, H, W, oh, ow, wy.shape[1], wx.shape[1], 0,
                                 stream_ptr()), "sst_bicubic")
    gd.check()
    ref = G.bicubic_taps(x.double(), wy, iy, wx, ix)
    terms = G.bicubic_taps(x.double(), wy.abs(), iy, wx.abs(), ix)
    G.assert_elementwise(f"bicubic {planes, H, W} x{scale}", y, ref, terms, wy.shape[1] + wx.shape[1] + 2)
    if scale == 0.25 and H % 4 == 0 and W % 4 == 0:               # the host path itself (rounded to the 1/255 grid) from the same taps
        host = bic(x.view(1, planes, H, W), scale)[0]
        assert float((torch.round(255 * ref) / 255 - host.double()).abs().max()) <= 1.0 / 255 + 1e-9
