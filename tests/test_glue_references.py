"""CPU: the hand-written fp64 formulas of tests/glue_refs.py against fp64 autograd / F.*, at a handful of the shapes the GPU suites
(test_bn_glue_fp64_gpu.py, test_misc_kernels_fp64_gpu.py) use them at - so a wrong reference cannot pass a wrong kernel."""
import pytest
import torch
import torch.nn.functional as F

import glue_refs as G
from conftest import rel_err

D = torch.float64
TIGHT = 1e-11                          # fp64 against fp64: re-association only


def _rand(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=D)


@pytest.mark.parametrize("act, slope_dev", [(1, True), (1, False), (0, False)])
@pytest.mark.parametrize("R, C", [(3, 4), (63, 16), (288, 64), (2305, 8)])
def test_bn_backward_coefficients_match_autograd(R, C, act, slope_dev):
    """S0 / S1 / S2 -> dgamma, dbeta, dslope and dy = cA gz + cB y + cC reproduce autograd of F.batch_norm(train) + PReLU / LeakyReLU;
    the [blk][3][C] partial layout sums to the same S."""
    y, up = _rand(R + C, R, C) * 2 + 3, _rand(R + C + 1, R, C)
    gamma, beta = _rand(C, C).abs() + 0.5, _rand(C + 1, C) * 0.3
    slope = torch.tensor([0.25], dtype=D) if slope_dev else 0.2
    auto = G.chain_grads(y, up, gamma, beta, slope, act, D)
    mean, var = G.batch_stats(y)
    assert rel_err(var, y.var(0, unbiased=False)) < TIGHT
    rstd = 1 / torch.sqrt(var + G.EPS)
    scale, shift = gamma * rstd, beta - mean * gamma * rstd
    S = G.bwd_sums(up, y, scale, shift, slope, act)
    for nblk in {1, G.reduce_blocks(R, C), min(R, 5)}:
        part = G.bwd_partials(up, y, scale, shift, slope, act, nblk)
        assert tuple(part.shape) == (nblk, 3, C) and rel_err(part.sum(0), S) < TIGHT
    co = G.bwd_coeffs(S, mean, rstd, gamma, R)
    gz = G.bwd_gz(up, y, scale, shift, slope, act)[0]
    assert rel_err(G.bwd_apply(gz, y, co["cA"], co["cB"], co["cC"]), auto["dy"]) < 1e-9
    assert rel_err(co["dgamma"], auto["dgamma"]) < 1e-9 and rel_err(co["dbeta"], auto["dbeta"]) < TIGHT
    if act and slope_dev:
        assert rel_err(co["dslope"], auto["dslope"]) < 1e-9


def test_bn_act_one_row_formula_is_batch_norm():
    """R = 1 takes the written-out formula (F.batch_norm refuses one value per channel): it is F.batch_norm's at R > 1."""
    y, gamma, beta = _rand(1, 7, 5), _rand(2, 5), _rand(3, 5)
    mean, var = G.batch_stats(y)
    z = (y - mean) / torch.sqrt(var + G.EPS) * gamma + beta
    assert rel_err(z, G.bn_act(y, gamma, beta, 0.2, 0)) < TIGHT
    assert torch.equal(G.bn_act(y[:1], gamma, beta, 0.2, 0), beta.expand(1, 5))
    g = G.chain_grads(y[:1], _rand(4, 1, 5), gamma, beta, torch.tensor([0.25], dtype=D), 1, D)
    assert float(g["dy"].abs().max()) == 0.0 and float(g["dgamma"].abs().max()) == 0.0


@pytest.mark.parametrize("groups", [2, 3])
def test_grouped_sums(groups):
    """Passes with their own statistics and shared parameters: dgamma / dbeta of the whole are the sums over the passes."""
    R, C = 40, 8
    gamma, beta = _rand(1, C).abs() + 0.5, _rand(2, C)
    ys = [_rand(10 + k, R, C) * 2.0 ** k + k for k in range(groups)]
    ups = [_rand(20 + k, R, C) for k in range(groups)]
    ga, be = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    sum(((G.bn_act(y, ga, be, 0.2, 1) * u).sum() for y, u in zip(ys, ups))).backward()
    per = [G.chain_grads(y, u, gamma, beta, 0.2, 1, D) for y, u in zip(ys, ups)]
    assert rel_err(sum(p["dgamma"] for p in per), ga.grad) < TIGHT and rel_err(sum(p["dbeta"] for p in per), be.grad) < TIGHT


def test_pixel_unshuffle_rows():
    B, H, W, C = 2, 4, 6, 3
    t = _rand(0, B * H * W, C)
    out = G.pixel_unshuffle_rows(t, B, H, W)
    v = t.view(B, H, W, C)
    for Y, X, c in ((0, 0, 0), (1, 0, 2), (2, 3, 1), (3, 5, 2)):
        assert torch.equal(out[:, Y // 2, X // 2, 4 * c + 2 * (Y & 1) + (X & 1)], v[:, Y, X, c])


@pytest.mark.parametrize("counts", [[1], [3, 0, 5, 1, 0, 7, 2], [4] * 6 + [0] * 3 + [9]])
def test_tiles_recombine_to_batch_statistics(counts):
    """make_tiles + Chan's combination give the statistics of the tensor; finalize_from gives nn.BatchNorm2d's running update."""
    R, C = sum(counts), 6
    y = _rand(R, R, C) + torch.arange(R, dtype=D).unsqueeze(1) * 0.1
    stats, cnt = G.make_tiles(y, counts)
    assert tuple(stats.shape) == (len(counts), 2, C) and cnt.tolist() == [float(c) for c in counts]
    n, mean, m2 = G.chan_combine(stats, cnt)
    assert float(n) == R and rel_err(mean, y.mean(0)) < TIGHT
    assert float((m2 - ((y - y.mean(0)) ** 2).sum(0)).abs().max()) < 1e-9
    if R > 1:
        gamma, beta = _rand(1, C), _rand(2, C)
        bn = torch.nn.BatchNorm2d(C, eps=G.EPS, momentum=G.MOMENTUM).double()
        with torch.no_grad():
            bn.weight.copy_(gamma), bn.bias.copy_(beta), bn.running_mean.copy_(_rand(3, C)), bn.running_var.copy_(_rand(4, C).abs())
        rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
        z = bn(y.t().reshape(1, C, R, 1))
        _, rstd, scale, shift, rm, rv = G.finalize_from(float(n), mean, m2, gamma, beta, rm0, rv0)
        assert rel_err((y * scale + shift).t().reshape(1, C, R, 1), z) < 1e-9
        assert rel_err(rm, bn.running_mean) < TIGHT and rel_err(rv, bn.running_var) < TIGHT
        bn.eval()
        es, et = G.eval_affine(gamma, beta, bn.running_mean, bn.running_var)
        assert rel_err((y * es + et).t().reshape(1, C, R, 1), bn(y.t().reshape(1, C, R, 1))) < 1e-9


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_pixel_loss_gradient(mode):
    x, gt = _rand(mode, 50).requires_grad_(True), _rand(mode + 9, 50)
    with torch.no_grad():
        gt[::7] = x[::7]
    G.pixel_loss(x, gt, mode).backward()
    assert torch.allclose(x.grad, G.pixel_loss_grad(x.detach(), gt, mode), rtol=1e-12, atol=0)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("affine, slope", [(True, 0.2), (True, 0.0), (False, 0.2)])
def test_feat_loss_gradient(affine, slope, mode):
    x, gt = _rand(1, 30, 6).requires_grad_(True), _rand(2, 30, 6)
    with torch.no_grad():
        gt.view(-1)[::5] = x.view(-1)[::5]
    sc, sh = (_rand(3, 6), _rand(4, 6)) if affine else (None, None)
    z = lambda v: F.leaky_relu(v * sc + sh if affine else v, slope)
    loss = (F.l1_loss if mode else F.mse_loss)(z(x), z(gt))
    assert rel_err(G.feat_loss(x.detach(), gt, sc, sh, slope, mode), loss) < TIGHT
    loss.backward()
    assert torch.allclose(x.grad, G.feat_loss_grad(x.detach(), gt, sc, sh, slope, mode), rtol=1e-12, atol=1e-18)


@pytest.mark.parametrize("t", [0.0, 1.0, 0.9])
def test_bce_formula(t):
    x = torch.tensor([100.0, -100.0, 20.0, -20.0, 0.0, 0.3, -2.0], dtype=D, requires_grad=True)
    loss = F.binary_cross_entropy_with_logits(x, torch.full_like(x, t))
    assert abs(float(loss.detach()) - float(G.bce_loss(x.detach(), t))) <= 1e-13 * float(loss.detach())
    loss.backward()
    assert torch.allclose(x.grad, G.bce_grad(x.detach(), t), rtol=1e-12, atol=1e-60)


def test_clamp_mask_is_clamp_backward():
    nan = float("nan")
    pre = torch.tensor([-0.0, 0.0, 1.0, 1.0000001, -1e-45, nan, 0.5, -3.0, 7.0], requires_grad=True)
    g = torch.arange(1.0, 10.0)
    pre.clamp(0, 1).backward(g)
    assert torch.equal(pre.grad, g * G.clamp_mask(pre.detach()))
    assert G.clamp_mask(pre.detach()).tolist() == [True, True, True, False, False, False, True, False, False]


def test_pool_rule_on_the_cpu():
    """What the pool kernels are held to: F.max_pool2d(F.relu(x), 2) lets a NaN through and sends it the gradient; the first maximum
    wins a tie; an all-negative window takes no gradient."""
    nan = float("nan")
    for w, out, grad in (([1.0, nan, 3.0, 2.0], nan, [0, 1, 0, 0]), ([-1.0, -2.0, nan, -3.0], nan, [0, 0, 1, 0]),
                         ([2.0, 2.0, 1.0, 2.0], 2.0, [1, 0, 0, 0]), ([-1.0, -2.0, -0.5, -3.0], 0.0, [0, 0, 0, 0]),
                         ([0.25, 0.75, 0.5, 0.75], 0.75, [0, 1, 0, 0])):
        x = torch.tensor(w).view(1, 1, 2, 2).requires_grad_(True)
        o = F.max_pool2d(F.relu(x), 2)
        o.backward(torch.ones_like(o))
        assert (o.item() != o.item()) if out != out else (o.item() == out)
        assert x.grad.flatten().tolist() == [float(v) for v in grad]


def test_bicubic_taps_is_the_host_path():
    from srganst.bicubic import Bicubic
    bic = Bicubic("cpu")
    x = torch.rand(1, 3, 24, 36, generator=torch.Generator().manual_seed(3))
    wy, iy, wx, ix = bic.tables(24, 36, 0.25, "cpu")
    ref = torch.round(255 * G.bicubic_taps(x[0], wy, iy, wx, ix)) / 255
    assert torch.equal(ref, bic(x, 0.25)[0])


def test_launch_geometry_mirrors():
    assert [G.reduce_blocks(R, 64) for R in (1, 3, 63, 288, 2305, 9216, 147456)] == [1, 1, 1, 3, 19, 72, 256]
    assert G.reduce_blocks(3, 1024) == 1 and G.reduce_blocks(9216, 1024) == 256 and G.reduce_blocks(9216, 4) == 5
    assert G.grid_for(1, 2048) == 1 and G.grid_for(257, 2048) == 2 and G.grid_for(10 ** 7, 2048) == 2048 and G.grid_for(10 ** 7, 1024) == 1024
    assert G.apply_fixed_c(256, 12) and not G.apply_fixed_c(100, 12) and G.apply_fixed_c(50, 64)


def test_elementwise_rule_catches_one_rounding_too_many():
    ref = torch.tensor([1.0, -2.0], dtype=D)
    G.assert_elementwise("ok", (ref * (1 + 2 * G.U24)).float(), ref, ref.abs(), 3)
    with pytest.raises(AssertionError):
        G.assert_elementwise("bad", ref * (1 + 8 * G.U24), ref, ref.abs(), 3)


def test_pinned_branches_only_where_fp32_cannot_decide():
    """bn_act with pin == 0 is F.prelu; undecided_signs pins nothing on well-conditioned data and only |z| within two fp32 roundings
    of the coefficients' size at |mean| / sigma = 1e3, where it takes the branch the fp32 coefficients give."""
    R, C = 500, 8
    y, up, gamma, beta = (_rand(1, R, C) + 0.3).float().double(), _rand(2, R, C), _rand(3, C).abs() + 0.5, _rand(4, C) * 0.3
    slope = torch.tensor([0.25], dtype=D)
    for offset in (0.0, 1000.0):
        yy = (y + offset).float().double()
        mean, var = G.batch_stats(yy)
        rstd = 1 / torch.sqrt(var + G.EPS)
        scale, shift = (gamma * rstd).float(), (beta - mean * gamma * rstd).float()
        z64 = G.bn_act(yy, gamma, beta, 0.0, 0)
        pin, n = G.undecided_signs(yy, scale, shift, z64)
        assert n == int((pin != 0).sum()) and n <= (0 if offset == 0 else R * C // 100)
        assert bool((z64[pin != 0].abs() <= 2 * G.U24 * 2100 * gamma.max()).all())
        a, b = G.chain_grads(yy, up, gamma, beta, slope, 1, D, pin=torch.zeros_like(pin)), G.chain_grads(yy, up, gamma, beta, slope, 1, D)
        assert all(torch.equal(a[k], b[k]) for k in a)
    z64[0, 0] = 1e-9
    forced = G.undecided_signs(torch.ones(1, 1, dtype=D), torch.tensor([1000.0]), torch.tensor([-1000.0]), z64[:1, :1])[0]
    assert forced.item() == -1                                  # the fp32 coefficients give z = 0: the negative branch
