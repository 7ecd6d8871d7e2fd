"""Validation metrics on the device: validate.image_metrics (tensor2img -> Y channel -> PSNR / SSIM) as one HIP kernel family
(csrc/metrics.hip: sst_image_metrics), rounding for rounding - not an approximation of the host path but the same numbers up to
fp64 summation order.  The kernel returns the MSE of Y (0..255 scale) and the mean SSIM per image; PSNR follows on the host from
the MSE (psnr_from_mse), after ONE device-to-host copy of all results.
lr_consistency is the LR-consistency number reported next to them: the per-image MSE of the re-downscaled output against the LR
input (csrc/bp_loss.hip, the forward of loss.BackProjectionLoss); lr_psnr_from_mse turns it into the LR-PSNR."""
from __future__ import annotations

import ctypes
import math

import torch
from torch import Tensor

from . import _abi
from ._abi import HipPathError

MIN_SIDE = 11          # the SSIM window; below it the valid region is empty (the host path then returns the mean of an empty map)


def workspace_doubles(B: int, H: int, W: int) -> int:
    n = ctypes.c_int64()
    _abi.check(_abi.lib().sst_image_metrics_workspace(B, H, W, ctypes.byref(n)), "sst_image_metrics_workspace")
    return n.value


def image_metrics_device(sr: Tensor, hr: Tensor, want_u8: bool = False, out: Tensor | None = None):
    """sr, hr: fp32 [B,3,H,W] RGB on one ROCm device -> fp64 [B,2] on that device: row b = (MSE of the Y channel of image b on the
    0..255 scale over all pixels, mean SSIM over the valid region), the values validate.image_metrics computes from.  With
    want_u8 also (sr_u8, hr_u8): uint8 [B,H,W,3] BGR = utils.tensor2img of each image.  `out`: write into this contiguous fp64
    [B,2] tensor (e.g. rows of a larger result buffer).  Runs on the current stream, no sync.  A NaN anywhere in sr or hr makes
    that image's row NaN (and its uint8 pixel 0)."""
    for name, t in (("sr", sr), ("hr", hr)):
        if not isinstance(t, Tensor) or not t.is_cuda:
            raise HipPathError(f"image_metrics_device: {name} must be a tensor on a ROCm device (no CPU fallback)")
        if t.dtype != torch.float32:
            raise HipPathError(f"image_metrics_device: {name} must be fp32, got {t.dtype}")
    if sr.dim() != 4 or sr.shape[1] != 3 or sr.shape != hr.shape or sr.device != hr.device:
        raise HipPathError(f"image_metrics_device: sr and hr must both be [B,3,H,W] on one device, got {tuple(sr.shape)} and "
                           f"{tuple(hr.shape)}")
    B, _, H, W = sr.shape
    if B < 1 or H < MIN_SIDE or W < MIN_SIDE:
        raise HipPathError(f"image_metrics_device: images of {W}x{H} are below the {MIN_SIDE}-px minimum of the SSIM window")
    sr, hr = sr.detach().contiguous(), hr.detach().contiguous()
    with torch.cuda.device(sr.device):
        if out is None:
            out = torch.empty(B, 2, dtype=torch.float64, device=sr.device)
        elif out.dtype != torch.float64 or tuple(out.shape) != (B, 2) or out.device != sr.device or not out.is_contiguous():
            raise HipPathError(f"image_metrics_device: out must be contiguous fp64 [{B}, 2] on {sr.device}")
        ws = torch.empty(workspace_doubles(B, H, W), dtype=torch.float64, device=sr.device)
        sr_u8 = hr_u8 = None
        if want_u8:
            sr_u8 = torch.empty(B, H, W, 3, dtype=torch.uint8, device=sr.device)
            hr_u8 = torch.empty(B, H, W, 3, dtype=torch.uint8, device=sr.device)
        _abi.check(_abi.lib().sst_image_metrics(_abi.ptr(sr), _abi.ptr(hr), B, H, W, _abi.ptr(out), _abi.ptr(sr_u8), _abi.ptr(hr_u8),
                                                _abi.ptr(ws), _abi.stream_ptr()), "sst_image_metrics")
    return (out, sr_u8, hr_u8) if want_u8 else out


_LR_TERMS = {}         # scale -> the lr-mode mse criterion whose tables and workspace lr_consistency uses


def lr_consistency(sr: Tensor, lr: Tensor, scale: int = 4, clamp: bool = True) -> Tensor:
    """sr fp32 [B,3,H,W] and its LR image lr fp32 [B,3,H/scale,W/scale] on one ROCm device -> fp64 [B] on that device: per image the
    MSE over RGB, on the 0..1 scale, of down(sr) against lr, down = the antialiased bicubic downscaling that makes LR inputs
    (loss.BackProjectionLoss's forward kernel, csrc/bp_loss.hip); clamp: sr is clamped to [0,1] first, as tensor2img does.  No
    gradient; runs on the current stream, no sync.  lr_psnr_from_mse turns a value into the LR-PSNR."""
    from .loss import BP_SCALES, BackProjectionLoss
    if scale not in BP_SCALES:
        raise HipPathError(f"lr_consistency: scale must be one of {BP_SCALES}, got {scale!r}")
    term = _LR_TERMS.get(scale)
    if term is None:
        term = _LR_TERMS[scale] = BackProjectionLoss(scale, "mse", target="lr")
    term._check(sr, lr, "lr_consistency")
    with torch.cuda.device(sr.device):
        _, per_image, _ = term._launch_fwd(sr.detach().contiguous(), lr.detach().contiguous(), False, per_image=True, clamp_sr=clamp)
    return per_image


def lr_psnr_from_mse(mse: float) -> float:
    """10 log10(1 / mse) for an MSE on the 0..1 scale (lr_consistency's)."""
    mse = float(mse)
    if mse == 0:
        return float("inf")
    return 10 * math.log10(1.0 / mse)


def psnr_from_mse(mse: float) -> float:
    """utils.PSNR's rule on the MSE of the 0..255 scale."""
    mse = float(mse)
    if mse == 0:
        return float("inf")
    return 20 * math.log10(255.0 / math.sqrt(mse))
