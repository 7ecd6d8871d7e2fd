"""The back-projection criterion's contract restated in plain torch (dtype-generic, dense tap matrices): what csrc/bp_loss.hip is
held to.

    My [oh,H], Mx [ow,W]   one axis of the antialiased bicubic downscaling as a dense matrix: bicubic._contribute's fp32 weights,
                           index_add'ed at their clamped indices (a border pixel collects every tap clamped onto it)
    down(x) = My @ x @ Mx^T,   D = down(sr) - T,   loss = mean |D| ("l1") or mean D^2 ("mse"); the gradient is autograd's

The target T is passed in, never recomputed in the evaluation's dtype: rounding ties of the 1/255 grid stay out of the fp64
comparison.  Also the shared inputs of tests/test_bp_refs.py, tests/test_bp_abi.py and tests/test_bp_loss_gpu.py: each case's images
and its fp32 / fp64 results are computed once and never modified."""
import functools

import torch

import ssim_refs

# name -> (B, H, W, scale, seed): see tests/test_bp_loss_gpu.py for why each is there.  Seeds: 100 + k where that seed keeps both
# margins below (tests/test_bp_refs.py asserts them), else the first seed found that does
CASES = {"one output": (2, 4, 4, 4, 100), "ragged": (2, 13, 22, 4, 101), "narrow": (1, 8, 100, 4, 102), "wide": (1, 8, 1100, 4, 240),
         "medium": (2, 48, 40, 4, 104), "x2": (2, 30, 26, 2, 206), "x8": (1, 64, 40, 8, 201), "crop": (2, 96, 96, 4, 112)}
NOISE = 0.08
# min |D| in the fp64 restatement that keeps fp32 and fp64 on one side of every L1 kink: about 50 x the largest fp32 error of D
# measured on the CPU (1.8e-7 - 2.4e-7)
L1_MARGIN = 1e-5
# min distance of 255 down(gt) from a rounding tie (k + 0.5) in fp64: 3 x that fp32 error on the 0..255 scale (2.4e-7 * 255 = 6e-5),
# so every fp32 evaluation of down(gt) rounds to the same grid point
TIE_MARGIN = 2e-4
L1_CASES = tuple(CASES)


@functools.lru_cache(maxsize=None)
def matrices(H, W, s):
    """-> (My [oh,H], Mx [ow,W]) in fp64, holding the fp32 weights exactly (a clamped duplicate adds up in fp64)."""
    from srganst.bicubic import _contribute
    out = []
    for n in (H, W):
        w, idx = _contribute(n, int(n * (1.0 / s)), 1.0 / s)
        M = torch.zeros(w.shape[0], n, dtype=torch.float64)
        for o in range(w.shape[0]):
            M[o].index_add_(0, idx[o], w[o].double())
        out.append(M)
    return tuple(out)


def down(x, s):
    """The downscaling in x's dtype."""
    My, Mx = (m.to(x.dtype) for m in matrices(x.shape[2], x.shape[3], s))
    return My @ x @ Mx.t()


def on_grid(t):
    return torch.round(255 * t) / 255


def bp_loss(sr, T, s, criterion="l1"):
    D = down(sr, s) - T.to(sr.dtype)
    return D.abs().mean() if criterion == "l1" else (D * D).mean()


def loss_and_grad(sr, T, s, criterion="l1", dtype=torch.float64):
    """-> (loss, d loss / d sr), both as fp64 tensors, evaluated in `dtype`."""
    x = sr.detach().clone().to(dtype).requires_grad_(True)              # a leaf of its own: the shared inputs stay as they are
    l = bp_loss(x, T, s, criterion)
    (g,) = torch.autograd.grad(l, x)
    return l.detach().double(), g.double()


def per_image_mse(sr, T, s):
    """fp64 [B]: the metric lr_consistency reports (without its clamp)."""
    D = down(sr.double(), s) - T.double()
    return (D * D).mean(dim=(1, 2, 3))


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> (sr, gt on the 1/255 grid, T_round, T_plain, s): T_round = the fp32 restatement of down(gt) rounded to the grid (the LR
    image), T_plain the same unrounded."""
    B, H, W, s, seed = CASES[name]
    sr, gt = ssim_refs.images(seed, B, H, W, NOISE)
    gt = ssim_refs.on_grid(gt)
    plain = down(gt, s)
    return sr, gt, on_grid(plain), plain, s


@functools.lru_cache(maxsize=None)
def case(name, criterion, rounded=True):
    """-> (sr, gt, T, s, l32, g32, l64, g64) of one table case: the fp32 and the fp64 evaluation of the restatement against T."""
    sr, gt, T_round, T_plain, s = inputs(name)
    T = T_round if rounded else T_plain
    l32, g32 = loss_and_grad(sr, T, s, criterion, torch.float32)
    l64, g64 = loss_and_grad(sr, T, s, criterion, torch.float64)
    return sr, gt, T, s, l32, g32, l64, g64


def min_abs_d(name):
    sr, _, T, _, s = inputs(name)
    return float((down(sr.double(), s) - T.double()).abs().min())


def tie_distance(name):
    _, gt, _, _, s = inputs(name)
    d = 255 * down(gt.double(), s)
    return float((d - torch.floor(d) - 0.5).abs().min())


def footprint(H, W, s, oy, ox):
    """bool [H,W]: the HR pixels under the taps of LR pixel (oy, ox)."""
    My, Mx = matrices(H, W, s)
    return (My[oy] != 0)[:, None] & (Mx[ox] != 0)[None, :]
