"""The SSIM criterion's contract restated in plain torch (dtype-generic, grouped conv2d): what csrc/ssim_loss.hip is held to.

    planes   "y":   P = (65.481 R + 128.553 G + 24.966 B + 16) / 255         "rgb": the three input planes
    window   w[i] = exp(-(i-5)^2 / (2 1.5^2)), i = 0..10, normalised in fp64; separable 'valid' correlation
    a = w(*)x, b = w(*)y, exx = w(*)x^2, eyy = w(*)y^2, exy = w(*)xy, C1 = k1^2, C2 = k2^2
    N1 = 2ab + C1, N2 = 2(exy - ab) + C2, D1 = a^2 + b^2 + C1, D2 = (exx - a^2) + (eyy - b^2) + C2, S = N1 N2 / (D1 D2)
    loss = 1 - mean(S) over batch, planes and valid positions; the gradient is taken with respect to sr only.

Also the shared inputs of tests/test_ssim_refs.py and tests/test_ssim_loss_gpu.py: each case's images and its fp32 / fp64 results
are computed once and never modified."""
import functools

import torch
import torch.nn.functional as F

LUMA = (65.481, 128.553, 24.966)

# name -> (B, H, W, noise): see tests/test_ssim_loss_gpu.py for why each is there
CASES = {"one window": (2, 11, 11, 0.08), "narrow": (2, 12, 43, 0.08), "medium": (2, 48, 40, 0.08),
         "anti-correlated": (3, 45, 33, 0.3), "ragged": (1, 75, 64, 0.02)}
SEED = 7


def images(seed, B, H, W, noise=0.08):
    """tests/test_st_general_gpu.py:_images - smooth texture (bicubic-upsampled noise) plus 0.05 N(0,1) for gt, gt + noise N(0,1) for
    sr, both clamped to [0, 1] -> (sr, gt)."""
    gen = torch.Generator().manual_seed(seed)
    base = torch.rand(B, 3, max(H // 6, 2), max(W // 6, 2), generator=gen)
    gt = F.interpolate(base, size=(H, W), mode="bicubic", align_corners=False)
    gt = (gt + 0.05 * torch.randn(gt.shape, generator=gen)).clamp(0, 1)
    x = (gt + noise * torch.randn(gt.shape, generator=gen)).clamp(0, 1)
    return x, gt


def on_grid(t):
    """The nearest image on the 1/255 grid (what utils.tensor2img keeps of a clamped image)."""
    return torch.round(t.clamp(0, 1) * 255.0) / 255.0


@functools.lru_cache(maxsize=None)
def window(dtype=torch.float64, device="cpu"):
    """The 11 taps, normalised in fp64 (kept per dtype and device: a second call copies nothing)."""
    i = torch.arange(11, dtype=torch.float64) - 5.0
    w = torch.exp(-(i * i) / (2.0 * 1.5 * 1.5))
    return (w / w.sum()).to(device=device, dtype=dtype)


def planes(t, channel):
    if channel == "rgb":
        return t
    if channel != "y":
        raise ValueError(channel)
    return (LUMA[0] * t[:, 0:1] + LUMA[1] * t[:, 1:2] + LUMA[2] * t[:, 2:3] + 16.0) / 255.0


def filt(p):
    """Separable 'valid' correlation of every plane of p [B,C,H,W] with the window -> [B,C,H-10,W-10]."""
    C = p.shape[1]
    w = window(p.dtype, p.device)
    p = F.conv2d(p, w.view(1, 1, 1, 11).expand(C, 1, 1, 11), groups=C)
    return F.conv2d(p, w.view(1, 1, 11, 1).expand(C, 1, 11, 1), groups=C)


def terms(sr, gt, channel="y", k1=0.01, k2=0.03):
    x, y = planes(sr, channel), planes(gt, channel)
    C1, C2 = k1 * k1, k2 * k2
    a, b, exx, eyy, exy = filt(x), filt(y), filt(x * x), filt(y * y), filt(x * y)
    N1, N2 = 2 * a * b + C1, 2 * (exy - a * b) + C2
    D1, D2 = a * a + b * b + C1, (exx - a * a) + (eyy - b * b) + C2
    return {"x": x, "y": y, "a": a, "b": b, "N1": N1, "N2": N2, "D1": D1, "D2": D2, "S": N1 * N2 / (D1 * D2)}


def ssim_map(sr, gt, channel="y", k1=0.01, k2=0.03):
    return terms(sr, gt, channel, k1, k2)["S"]


def ssim_loss(sr, gt, channel="y", k1=0.01, k2=0.03):
    return 1 - ssim_map(sr, gt, channel, k1, k2).mean()


def loss_and_grad(sr, gt, channel="y", dtype=torch.float64, k1=0.01, k2=0.03):
    """-> (loss, d loss / d sr), both as fp64 tensors, evaluated in `dtype`."""
    x = sr.to(dtype).requires_grad_(True)
    l = ssim_loss(x, gt.to(dtype), channel, k1, k2)
    (g,) = torch.autograd.grad(l, x)
    return l.detach().double(), g.double()


def full_corr(G):
    """w (*)T G: the adjoint of filt - a full correlation with the symmetric window, zero outside the valid region."""
    return filt(F.pad(G, (10, 10, 10, 10)))


def grad_from_maps(sr, gt, channel="y", k1=0.01, k2=0.03):
    """d loss / d sr through the three maps the kernels use, formed without dividing by N1 or N2:
    Ga = dS/da, Gxx = dS/dexx = -N1 N2 / (D1 D2^2), Gxy = dS/dexy = 2 N1 / (D1 D2)."""
    t = terms(sr, gt, channel, k1, k2)
    a, b, N1, N2, D1, D2, S = (t[k] for k in ("a", "b", "N1", "N2", "D1", "D2", "S"))
    iD = 1 / (D1 * D2)
    Ga = 2 * b * (N2 - N1) * iD - 2 * a * S * (D2 - D1) * iD
    Gxx, Gxy = -S / D2, 2 * N1 * iD
    dP = -(full_corr(Ga) + 2 * t["x"] * full_corr(Gxx) + t["y"] * full_corr(Gxy)) / S.numel()
    if channel == "rgb":
        return dP
    return torch.cat([dP * (c / 255.0) for c in LUMA], dim=1)


def n2_negative_fraction(sr, gt, channel="y"):
    return float((terms(sr.double(), gt.double(), channel)["N2"] < 0).double().mean())


@functools.lru_cache(maxsize=None)
def case(name, channel):
    """-> (sr, gt, l32, g32, l64, g64) of one table case: the fp32 and the fp64 evaluation of the restatement."""
    B, H, W, noise = CASES[name]
    x, gt = images(SEED, B, H, W, noise)
    l32, g32 = loss_and_grad(x, gt, channel, torch.float32)
    l64, g64 = loss_and_grad(x, gt, channel, torch.float64)
    return x, gt, l32, g32, l64, g64
