"""The focal frequency loss's contract restated in plain torch (dtype-generic, torch.fft): what csrc/freq_loss.hip is held to.  The
published implementation's defaults (Jiang et al., ICCV 2021): one patch per image, no averaged spectrum, no log weights, per-plane
normalisation.

    d = sr - gt per image and RGB plane;  D = fft2(d, norm="ortho");  e = |D|^2 = Re^2 + Im^2
    w = sqrt(e)^alpha / max over the plane's H x W frequencies of sqrt(e)^alpha;  NaN -> 0, clamped to [0, 1], detached
    loss = mean over batch, planes and frequencies of w e;   the gradient is taken with respect to sr only:
    d loss / d sr = 2 / (B 3 H W) Re(ifft2(w .* D, norm="ortho"))

Also the shared inputs of tests/test_freq_refs.py and tests/test_freq_loss_gpu.py: each case's images and its fp32 / fp64 results are
computed once and never modified."""
import functools
import math

import torch
import torch.nn.functional as F

# name -> (B, H, W): the smallest shapes at which the kernels can go wrong; see tests/test_freq_loss_gpu.py for why each is there
CASES = {"pixel": (2, 1, 1), "row": (1, 1, 7), "column": (1, 6, 1), "even": (2, 12, 10), "odd": (2, 45, 33), "mixed": (1, 48, 37),
         "ragged": (1, 75, 64), "crop": (2, 96, 96), "tall": (1, 130, 18), "longest": (1, 512, 5), "dominant": (2, 40, 36)}
SEED = 11
NOISE = 0.08


def images(seed, B, H, W, noise=NOISE):
    """A smooth gt in 0..1 (bicubic-upsampled noise, clamped) and sr = gt + noise N(0,1) -> (sr, gt)."""
    gen = torch.Generator().manual_seed(seed)
    base = torch.rand(B, 3, max(H // 6, 2), max(W // 6, 2), generator=gen)
    gt = F.interpolate(base, size=(H, W), mode="bicubic", align_corners=False).clamp(0, 1)
    x = gt + noise * torch.randn(gt.shape, generator=gen)
    return x, gt


def case_images(name):
    B, H, W = CASES[name]
    if name == "dominant":                               # d = 0.2 + 0.01 N(0,1): DC carries the maximum, the weights span many decades
        _, gt = images(SEED, B, H, W)
        gen = torch.Generator().manual_seed(SEED + 1)
        return gt + (0.2 + 0.01 * torch.randn(gt.shape, generator=gen)), gt
    return images(SEED, B, H, W)


def weights(e, alpha):
    """The per-plane normalised spectrum weight of e [B,C,H,W] (detached)."""
    s = torch.sqrt(e) ** alpha
    w = s / s.amax(dim=(-2, -1), keepdim=True)
    w = torch.where(torch.isnan(w), torch.zeros_like(w), w)
    return w.clamp(0.0, 1.0).detach()


def freq_loss(sr, gt, alpha=1.0):
    D = torch.fft.fft2(sr - gt, norm="ortho")
    e = D.real ** 2 + D.imag ** 2
    return (weights(e, alpha) * e).mean()


def freq_loss_stacked(sr, gt, alpha=1.0):
    """A second writing, as the published code has it: real and imaginary parts stacked in a last dimension, the squared distance of
    the two spectra (not the spectrum of the difference), the weight from the flattened plane's maximum."""
    def spec(t):
        f = torch.fft.fft2(t, norm="ortho")
        return torch.stack([f.real, f.imag], -1)
    diff = (spec(sr) - spec(gt)) ** 2
    dist = diff[..., 0] + diff[..., 1]
    m = torch.sqrt(dist) ** alpha
    m = m / m.flatten(-2).max(-1).values[..., None, None]
    m[torch.isnan(m)] = 0.0
    m = torch.clamp(m, min=0.0, max=1.0).clone().detach()
    return torch.mean(m * dist)


def loss_and_grad(sr, gt, alpha=1.0, dtype=torch.float64):
    """-> (loss, d loss / d sr) by autograd, both as fp64 tensors, evaluated in `dtype`."""
    x = sr.to(dtype).requires_grad_(True)
    l = freq_loss(x, gt.to(dtype), alpha)
    (g,) = torch.autograd.grad(l, x)
    return l.detach().double(), g.double()


def grad_closed_form(sr, gt, alpha=1.0):
    """2 / (B 3 H W) Re(F^H (w .* D)): what the backward kernels compute."""
    D = torch.fft.fft2(sr - gt, norm="ortho")
    w = weights(D.real ** 2 + D.imag ** 2, alpha)
    return 2.0 / sr.numel() * torch.fft.ifft2(w * D, norm="ortho").real


def cosine(A, u, v, H, W, dtype=torch.float64):
    """A cos(2 pi (u x / W + v y / H)) as one [H, W] plane."""
    y = torch.arange(H, dtype=torch.float64).view(H, 1)
    x = torch.arange(W, dtype=torch.float64).view(1, W)
    return (A * torch.cos(2.0 * math.pi * (u * x / W + v * y / H))).to(dtype)


def cosine_value(A, u, v, H, W):
    """The plane's loss for d = cosine(A, u, v): A^2 / 2, and A^2 when (u, v) is its own negative (DC, or Nyquist on both axes)."""
    own_negative = (2 * u) % W == 0 and (2 * v) % H == 0
    return A * A if own_negative else A * A / 2.0


@functools.lru_cache(maxsize=None)
def case(name, alpha=1.0):
    """-> (sr, gt, l32, g32, l64, g64) of one table case: the fp32 and the fp64 evaluation of the restatement."""
    x, gt = case_images(name)
    l32, g32 = loss_and_grad(x, gt, alpha, torch.float32)
    l64, g64 = loss_and_grad(x, gt, alpha, torch.float64)
    return x, gt, l32, g32, l64, g64
