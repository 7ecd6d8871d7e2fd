"""Plain-torch restatements of the BatchNorm / activation glue (csrc/bn_elem.hip) and of the small criterion and layout kernels
(csrc/misc.hip), one formula per op as in include/srganst.h and the kernel header comments.  Every function takes the dtype of its
inputs: run in fp64 it is the truth of tests/test_bn_glue_fp64_gpu.py and tests/test_misc_kernels_fp64_gpu.py, run in fp32 it is the
"same formula in fp32" of conftest.assert_fp64_truth.  tests/test_glue_references.py holds these formulas to fp64 autograd / F.* on the
CPU, so a wrong formula here cannot pass a wrong kernel.  Tensors are [R rows, C channels] (NHWC flattened) unless said otherwise."""
import torch
import torch.nn.functional as F

EPS, MOMENTUM = 1e-5, 0.1
U24 = 2.0 ** -24                      # unit roundoff of fp32: one rounding moves a value by at most U24 * |value|
F32_MIN_NORMAL = 2.0 ** -126


# ------------------------------------------------------------------------------------------------ launch geometry (host mirrors)
def grid_for(items, cap):
    """grid_for() of bn_elem.hip (cap 2048) and misc.hip (cap 1024): workgroups of 256 threads."""
    return max(1, min(cap, (items + 255) // 256))


def reduce_blocks(R, C):
    """sst_bwd_reduce_blocks."""
    return max(1, min((R * (C // 4) + 2047) // 2048, 256, R))


def apply_fixed_c(R, C):
    """bwd_apply_kernel: `fixed_c = stride % c4n == 0` with stride = gridDim.x * 256."""
    return (grid_for(R * (C // 4), 2048) * 256) % (C // 4) == 0


# ------------------------------------------------------------------------------------------------ BatchNorm + activation
def slope_act(z, slope):
    return torch.where(z > 0, z, z * slope)


def bn_act(y, gamma, beta, slope, act, eps=EPS, pin=None):
    """Train-mode BatchNorm over the rows of y [R, C], then PReLU (slope: 1-element tensor) / LeakyReLU (slope: float) when act.
    F.batch_norm refuses one value per channel, so R = 1 takes the written-out formula (same value: test_glue_references).
    pin [R, C] (+1 / -1 / 0): elements whose activation branch is given (positive / negative) instead of read off the sign of z -
    see undecided_signs; where pin == 0 this is F.prelu / F.leaky_relu."""
    if y.shape[0] > 1:
        z = F.batch_norm(y, None, None, gamma, beta, True, 0.0, eps)
    else:
        mean = y.mean(0)
        z = (y - mean) / torch.sqrt(((y - mean) ** 2).mean(0) + eps) * gamma + beta
    if not act:
        return z
    if pin is not None:
        return torch.where(torch.where(pin == 0, z > 0, pin > 0), z, z * slope)
    return F.prelu(z, slope) if torch.is_tensor(slope) else F.leaky_relu(z, slope)


def undecided_signs(y, scale32, shift32, z64):
    """The activation branch of an element is read off the sign of z = y*scale + shift with fp32 scale / shift (include/srganst.h).
    Each of the two is one rounding away from its fp64 value, so z sits within 2^-24 (|y scale| + |shift|) of the fp64 z64, and where
    |z64| is below TWICE that the sign is not decided by the fp32 coefficients: no kernel that takes them can be held to either
    branch.  Returns pin for bn_act: on those elements the branch the fp32 coefficients give (their exact product-sum, the sign
    fmaf keeps), 0 elsewhere - and asserts that elsewhere that branch IS the fp64 one."""
    zk = y * scale32.double() + shift32.double()
    undecided = z64.abs() <= 2 * U24 * ((y * scale32.double()).abs() + shift32.double().abs())
    assert not bool((((zk > 0) != (z64 > 0)) & ~undecided).any()), "fp32 scale / shift flip a sign that fp32 decides"
    pin = torch.where(zk > 0, 1, -1) * undecided
    return pin, int(undecided.sum())


def chain_grads(y, up, gamma, beta, slope, act, dtype, eps=EPS, pin=None):
    """Autograd of bn_act in `dtype` against the upstream gradient `up` -> dict(dy, dgamma, dbeta[, dslope])."""
    y, gamma, beta = (t.detach().to(dtype).clone().requires_grad_(True) for t in (y, gamma, beta))
    leaves = {"dy": y, "dgamma": gamma, "dbeta": beta}
    if torch.is_tensor(slope):
        slope = slope.detach().to(dtype).clone().requires_grad_(True)
        if act:
            leaves["dslope"] = slope
    bn_act(y, gamma, beta, slope, act, eps, pin).backward(up.to(dtype))
    return {k: v.grad.detach() for k, v in leaves.items()}


def batch_stats(y):
    """(mean, biased variance) over the rows."""
    mean = y.mean(0)
    return mean, ((y - mean) ** 2).mean(0)


def bwd_gz(g, y, scale, shift, slope, act):
    """z = y*scale + shift (z = y when scale is None), gz = g * act'(z); also g * min(z, 0) (the slope gradient's summand)."""
    z = y if scale is None else y * scale + shift
    if not act:
        return g, torch.zeros_like(g)
    return g * torch.where(z > 0, torch.ones_like(z), torch.ones_like(z) * slope), g * z.clamp(max=0)


def bwd_sums(g, y, scale, shift, slope, act):
    """-> [3, C]: sum gz, sum gz*y, sum g*min(z,0) over the rows."""
    gz, gm = bwd_gz(g, y, scale, shift, slope, act)
    return torch.stack([gz.sum(0), (gz * y).sum(0), gm.sum(0)])


def bwd_partials(g, y, scale, shift, slope, act, nblk):
    """The [blk][3][C] layout bwd_reduce_kernel writes: block b owns rows [b*rpb, min(R, (b+1)*rpb)), rpb = ceil(R / nblk)."""
    R = y.shape[0]
    rpb = (R + nblk - 1) // nblk
    sc = lambda b: slice(b * rpb, min(R, (b + 1) * rpb))
    return torch.stack([bwd_sums(g[sc(b)], y[sc(b)], scale, shift, slope, act) for b in range(nblk)])


def bwd_coeffs(S, mean, rstd, gamma, n):
    """bwd_finalize: from S = [3, C] -> dict(dgamma, dbeta, dslope, cA, cB, cC) with dy = cA*gz + cB*y + cC."""
    sgh = rstd * (S[1] - mean * S[0])
    m1, m2, a = S[0] / n, sgh / n, gamma * rstd
    return {"dgamma": sgh, "dbeta": S[0], "dslope": S[2].sum().reshape(1), "cA": a, "cB": -a * rstd * m2,
            "cC": -a * m1 + a * rstd * mean * m2}


def bwd_apply(gz, y, cA, cB, cC):
    return cA * gz + cB * y + cC


def pixel_unshuffle_rows(t, B, H, W):
    """[B*H*W, C] rows of the shuffled tensor -> the pre-PixelShuffle(2) tensor [B, H/2, W/2, 4C] (stored channel 4c + 2(Y&1) + (X&1))."""
    C = t.shape[-1]
    return F.pixel_unshuffle(t.view(B, H, W, C).permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------------ forward statistics
def make_tiles(y, counts):
    """Cuts the rows of y [R = sum(counts), C] into consecutive tiles -> stats [ntiles, 2, C] = (sum, sum (x - tile mean)^2), cnt."""
    counts = torch.as_tensor(counts, dtype=torch.int64)
    nt, C = counts.numel(), y.shape[1]
    tid = torch.repeat_interleave(torch.arange(nt), counts)
    s = torch.zeros(nt, C, dtype=y.dtype).index_add_(0, tid, y)
    tmean = s / counts.clamp_min(1).to(y.dtype).unsqueeze(1)
    m2 = torch.zeros(nt, C, dtype=y.dtype).index_add_(0, tid, (y - tmean[tid]) ** 2)
    return torch.stack([s, m2], 1).contiguous(), counts.to(y.dtype)


def chan_combine(stats, cnt):
    """Chan et al. combination of the tiles, as bn_finalize_kernel: -> (n, mean, M2)."""
    n = cnt.sum()
    mean = stats[:, 0].sum(0) / n
    ok = cnt > 0
    d = stats[ok, 0] / cnt[ok].unsqueeze(1) - mean
    return n, mean, (stats[ok, 1] + cnt[ok].unsqueeze(1) * d * d).sum(0)


def finalize_from(n, mean, m2, gamma, beta, run_mean=None, run_var=None, eps=EPS, momentum=MOMENTUM):
    """(mean, rstd, scale, shift, run_mean', run_var') from the count, mean and sum of squared deviations of a batch."""
    rstd = 1 / torch.sqrt(m2 / n + eps)
    scale = gamma * rstd
    out = [mean, rstd, scale, beta - mean * scale, None, None]
    if run_mean is not None:
        out[4] = (1 - momentum) * run_mean + momentum * mean
        out[5] = (1 - momentum) * run_var + momentum * (m2 / max(float(n) - 1, 1.0))      # unbiased, as nn.BatchNorm2d
    return out


def eval_affine(gamma, beta, run_mean, run_var, eps=EPS):
    scale = gamma / torch.sqrt(run_var + eps)
    return scale, beta - run_mean * scale


# ------------------------------------------------------------------------------------------------ criteria
def relu_if(t, on):
    return F.relu(t) if on else t


def pixel_loss(x, gt, mode):
    """mode & 1: 0 = MSE, 1 = L1; mode & 2: on relu(x), relu(gt)."""
    a, b = relu_if(x, mode & 2), relu_if(gt, mode & 2)
    return F.l1_loss(a, b) if mode & 1 else F.mse_loss(a, b)


def pixel_loss_grad(x, gt, mode):
    """d pixel_loss / dx written out."""
    d = relu_if(x, mode & 2) - relu_if(gt, mode & 2)
    g = (torch.sign(d) if mode & 1 else 2 * d) / x.numel()
    return g * (x > 0) if mode & 2 else g


def feat_act(v, scale, shift, slope):
    z = v if scale is None else v * scale + shift
    return z, slope_act(z, slope)


def feat_loss(x, gt, scale, shift, slope, mode):
    """crit(lrelu(x*s + t) - lrelu(gt*s + t)) over [rows, C]."""
    a, b = feat_act(x, scale, shift, slope)[1], feat_act(gt, scale, shift, slope)[1]
    return F.l1_loss(a, b) if mode else F.mse_loss(a, b)


def feat_loss_grad(x, gt, scale, shift, slope, mode):
    za, a = feat_act(x, scale, shift, slope)
    d = a - feat_act(gt, scale, shift, slope)[1]
    g = (torch.sign(d) if mode else 2 * d) / x.numel()
    g = g * torch.where(za > 0, torch.ones_like(za), torch.ones_like(za) * slope)
    return g if scale is None else g * scale


def bce_loss(x, t):
    """mean of max(x,0) - x t + log1p(exp(-|x|))."""
    return (x.clamp(min=0) - x * t + torch.log1p(torch.exp(-x.abs()))).mean()


def bce_grad(x, t):
    return (torch.sigmoid(x) - t) / x.numel()


def clamp_mask(pre):
    return (pre >= 0) & (pre <= 1)


def bicubic_taps(x, wy, iy, wx, ix):
    """x [planes, H, W] -> [planes, oh, ow]: vertical taps first, then horizontal (srganst/bicubic.py's host path without the 1/255 grid)."""
    v = (x[:, iy, :] * wy.to(x.dtype).unsqueeze(0).unsqueeze(3)).sum(2)                       # [planes, oh, W]
    return (v[:, :, ix] * wx.to(x.dtype).unsqueeze(0).unsqueeze(1)).sum(3)                    # [planes, oh, ow]


# ------------------------------------------------------------------------------------------------ checks
def assert_elementwise(name, hip, ref64, terms64, k):
    """Elementwise fp32 chain: |hip - ref64| <= k * 2^-24 * sum|terms| per element, k = fp32 roundings of the kernel's expression."""
    hip, ref64, terms64 = hip.detach().cpu().double(), ref64.double(), terms64.double()
    assert hip.shape == ref64.shape, (name, hip.shape, ref64.shape)
    assert bool(torch.isfinite(hip).all()), f"{name}: non-finite output"
    excess = (hip - ref64).abs() - k * U24 * terms64 - F32_MIN_NORMAL      # below the smallest normal number fp32 has no relative precision
    worst = float(((hip - ref64).abs() / (U24 * terms64).clamp_min(1e-300)).max()) if hip.numel() else 0.0
    assert bool((excess <= 0).all()), f"{name}: {int((excess > 0).sum())} elements off by more than {k} roundings (worst {worst:.2f})"
    return worst


def assert_scalar_truth(name, hip, ref32, ref64, report=None):
    """conftest.assert_fp64_truth for one number; a truth below the smallest normal fp32 number carries no relative precision in the
    format, there the error is held to that number instead."""
    from conftest import assert_fp64_truth
    hip, ref32, ref64 = (torch.as_tensor(v).detach().cpu().double().reshape(1) for v in (hip, ref32, ref64))
    if abs(float(ref64)) < F32_MIN_NORMAL:
        assert abs(float(hip) - float(ref64)) <= F32_MIN_NORMAL, f"{name}: {float(hip):.3e} against a subnormal truth {float(ref64):.3e}"
        return
    assert_fp64_truth(name, hip, ref32, ref64, report)


def print_report(title, report):
    if report:
        print(f"\n[{title}] worst |hip - fp64| (rel) per quantity, next to the fp32 reference's own error")
        worst = {}
        for name, e_hip, e_32 in report:
            key = name.split(" ")[0]
            if key not in worst or e_hip > worst[key][0]:
                worst[key] = (e_hip, e_32, name)
        for key, (e_hip, e_32, name) in worst.items():
            print(f"  {key:12s} hip {e_hip:.3e}   fp32 ref {e_32:.3e}   ({name})")


# ------------------------------------------------------------------------------------------------ guard bands (GPU tests only)
SENTINEL = -1.2345678e30
GUARD = 256                           # floats on either side (a multiple of 4: the 16-byte stores of the kernels stay aligned)


class Guarded:
    """Outputs carved out of larger buffers pre-filled with a sentinel; check() asserts that the bands before and after every output
    are untouched, which catches out-of-range stores without causing any.  patch(ops) routes the allocations the srganst.ops wrappers
    make themselves (_f32, torch.empty_like) through here for the length of a `with` block."""

    def __init__(self, device="cuda"):
        self.device, self.bufs = device, []

    def empty(self, *shape, dtype=torch.float32, fill=None):
        shape = tuple(shape[0]) if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)) else tuple(shape)
        n = 1
        for s in shape:
            n *= int(s)
        assert dtype in (torch.float32, torch.int32)
        buf = torch.full((n + 2 * GUARD,), SENTINEL, device=self.device, dtype=torch.float32)
        self.bufs.append((buf, n))
        out = buf[GUARD:GUARD + n].view(dtype).view(shape)
        if fill is not None:
            out.fill_(fill)
        return out

    def put(self, t):
        """A guarded device copy of a host tensor (for outputs that are accumulated onto)."""
        out = self.empty(t.shape)
        out.copy_(t.to(torch.float32))
        return out

    def check(self):
        torch.cuda.synchronize()
        for i, (buf, n) in enumerate(self.bufs):
            assert bool((buf[:GUARD] == SENTINEL).all()), f"guard band before output {i} ({n} floats) was written"
            assert bool((buf[GUARD + n:] == SENTINEL).all()), f"guard band after output {i} ({n} floats) was written"
        self.bufs = []

    def patch(self, ops):
        return _Patch(self, ops)


class _TorchProxy:
    def __init__(self, guarded):
        self._g = guarded

    def empty_like(self, t, **kw):
        return self._g.empty(t.shape)

    def __getattr__(self, name):
        return getattr(torch, name)


class _Patch:
    def __init__(self, guarded, ops):
        self.g, self.ops = guarded, ops

    def __enter__(self):
        self.saved = (self.ops._f32, self.ops.torch)
        self.ops._f32 = lambda *shape, like: self.g.empty(*shape)
        self.ops.torch = _TorchProxy(self.g)
        return self.g

    def __exit__(self, *exc):
        self.ops._f32, self.ops.torch = self.saved
        if exc[0] is None:
            self.g.check()
        return False
