"""The contracts of GradientLoss and GradientVarianceLoss restated in plain torch (dtype-generic: conv2d, unfold, var): what
csrc/grad_loss.hip is held to.

    Gv, Gh   F.conv2d(plane, K, padding=1) with the vertical operator K - "central" [[0,-1,0],[0,0,0],[0,1,0]], "sobel"
             [[-1,-2,-1],[0,0,0],[1,2,1]] - and with its transpose: pixels outside the image count as zero
    GradientLoss           per image and RGB plane M(I) = sqrt(Gv(I)^2 + Gh(I)^2 + eps); mean |M(sr) - M(gt)| ("l1") or of its square
                           ("mse") over B*3*H*W; torch's abs has derivative 0 at a tie
    GradientVarianceLoss   gray = 0.2989 R + 0.587 G + 0.114 B; its Sobel responses cut into non-overlapping p x p patches from the
                           top-left corner (unfold with stride p drops leftover rows and columns); v = the unbiased variance of a
                           patch; mean((vv(sr) - vv(gt))^2) + mean((vh(sr) - vh(gt))^2)
    the gradient is taken with respect to sr only.

Also the shared inputs of tests/test_grad_refs.py and tests/test_grad_loss_gpu.py: each case's images and its fp32 / fp64 results
are computed once and never modified.  The images stay strictly inside (0, 1) without a clamp (a clamped pair coincides over whole
neighbourhoods, where the "l1" criterion sits on its kink); the seeds of the GradientLoss cases were searched until min |M(sr) -
M(gt)| >= 1e-5 in fp64 for both operators (tests/test_grad_refs.py asserts it), so the sign of no position depends on the precision."""
import functools

import torch
import torch.nn.functional as F

OPERATORS = {"central": [[0.0, -1.0, 0.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0]],
             "sobel": [[-1.0, -2.0, -1.0], [0.0, 0.0, 0.0], [1.0, 2.0, 1.0]]}
GRAY = (0.2989, 0.587, 0.114)

# name -> (seed, B, H, W): see tests/test_grad_loss_gpu.py for why each is there
GRAD_CASES = {"single row": (1, 2, 1, 7), "seams": (35, 2, 33, 65), "medium": (1, 2, 48, 40), "ragged": (264, 1, 75, 64)}
# name -> (seed, B, H, W, patch)
GV_CASES = {"one patch": (11, 2, 8, 8, 8), "leftover": (12, 2, 19, 43, 8), "tile of 30": (13, 1, 31, 34, 3), "p5": (14, 1, 75, 64, 5),
            "p32": (15, 1, 64, 40, 32), "p2": (16, 1, 9, 5, 2), "medium": (17, 2, 48, 40, 8)}


def images(seed, B, H, W, noise=0.08):
    """gt: a smooth field in [0.15, 0.85] (bilinearly upsampled uniform noise) plus uniform noise of +-0.02; sr: gt plus uniform noise
    of +-`noise`.  Both stay inside [0.05, 0.95] by construction: no clamp -> (sr, gt)."""
    gen = torch.Generator().manual_seed(seed)
    base = torch.rand(B, 3, max(H // 6, 2), max(W // 6, 2), generator=gen)
    smooth = F.interpolate(base, size=(H, W), mode="bilinear", align_corners=True)
    gt = 0.15 + 0.7 * smooth + 0.02 * (2 * torch.rand(smooth.shape, generator=gen) - 1)
    x = gt + noise * (2 * torch.rand(gt.shape, generator=gen) - 1)
    return x, gt


@functools.lru_cache(maxsize=None)
def kernels(operator, dtype=torch.float64, device="cpu"):
    """(Kv, Kh) as [1,1,3,3] (kept per dtype and device: a second call copies nothing, so a call can be captured into a graph)."""
    kv = torch.tensor(OPERATORS[operator], dtype=dtype)
    return tuple(k.contiguous().view(1, 1, 3, 3).to(device) for k in (kv, kv.t()))


def responses(p, operator):
    """(Gv, Gh) of every plane of p [B,C,H,W]: zero-padded 3x3 correlations with the vertical operator and its transpose."""
    C = p.shape[1]
    return tuple(F.conv2d(p, k.expand(C, 1, 3, 3), padding=1, groups=C) for k in kernels(operator, p.dtype, p.device))


def magnitude(p, operator="central", eps=1e-6):
    gv, gh = responses(p, operator)
    return torch.sqrt(gv * gv + gh * gh + eps)


def gradient_loss(sr, gt, operator="central", criterion="l1", eps=1e-6):
    d = magnitude(sr, operator, eps) - magnitude(gt, operator, eps)
    if criterion == "l1":
        return d.abs().mean()
    if criterion != "mse":
        raise ValueError(criterion)
    return (d * d).mean()


def gray(t):
    return GRAY[0] * t[:, 0:1] + GRAY[1] * t[:, 1:2] + GRAY[2] * t[:, 2:3]


def patch_variances(t, patch):
    """(vv, vh) [B, (H//patch) * (W//patch)]: the unbiased variance of every patch of the gray Sobel responses of t [B,3,H,W]."""
    return tuple(F.unfold(g, patch, stride=patch).var(dim=1, unbiased=True) for g in responses(gray(t), "sobel"))


def gv_loss(sr, gt, patch=8):
    (vx, hx), (vy, hy) = patch_variances(sr, patch), patch_variances(gt, patch)
    return ((vx - vy) ** 2).mean() + ((hx - hy) ** 2).mean()


def loss_and_grad(fn, sr, gt, dtype=torch.float64):
    """fn(sr, gt) -> 0-dim, evaluated in `dtype` -> (loss, d loss / d sr), both as fp64 tensors."""
    x = sr.to(dtype).requires_grad_(True)
    l = fn(x, gt.to(dtype))
    (g,) = torch.autograd.grad(l, x)
    return l.detach().double(), g.double()


def _both(fn, x, gt):
    return (x, gt, *loss_and_grad(fn, x, gt, torch.float32), *loss_and_grad(fn, x, gt, torch.float64))


@functools.lru_cache(maxsize=None)
def case(name, operator=None, criterion=None):
    """-> (sr, gt, l32, g32, l64, g64) of one table case: the fp32 and the fp64 evaluation of the restatement.  A GradientLoss case
    takes its operator and criterion, a GradientVarianceLoss case (GV_CASES; its patch size is in the table) neither."""
    if operator is None:
        seed, B, H, W, patch = GV_CASES[name]
        return _both(lambda a, b: gv_loss(a, b, patch), *images(seed, B, H, W))
    seed, B, H, W = GRAD_CASES[name]
    return _both(lambda a, b: gradient_loss(a, b, operator, criterion), *images(seed, B, H, W))


def min_magnitude_gap(name, operator):
    """min |M(sr) - M(gt)| of a GradientLoss case in fp64: how far its nearest position is from the kink of |.|."""
    seed, B, H, W = GRAD_CASES[name]
    x, gt = images(seed, B, H, W)
    return float((magnitude(x.double(), operator) - magnitude(gt.double(), operator)).abs().min())
