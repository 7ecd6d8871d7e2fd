"""Validation / test path.  Mirrors reference validate.py:18-137: batch-1 full-image generator forward
under no_grad -> tensor2img -> /255 -> Y channel -> PSNR / SSIM (no border shave), mean +- CI.
The generator forward is the HIP path in eval mode (BatchNorm folded to scale/shift from running stats).
With config.DATA.VALIDATE_ON_DEVICE (or on_device=True) the metrics are taken on the device too (metrics.py).
With config.DATA.VALIDATE_ST (or with_st=True, or --st) every image also gets its structure-tensor distance (st.st_distance): the
quantity the ``ST`` criterion optimises, reported next to PSNR and SSIM.
With config.DATA.VALIDATE_TILE = T > 0 (or tile=T, or --tile T) the generator runs tiled (upscale.Upscaler, windows of T LR pixels with
the exact halo): test images of any size, the whole-image forward's result.
With config.DATA.VALIDATE_LR (or with_lr=True, or --lr-consistency) every image also gets its LR consistency (metrics.lr_consistency:
the generator's output, clamped and downscaled again by the kernel that made the LR input, against that LR input) as an ``LR-PSNR``
column: the quantity the ``BackProjection`` criterion optimises.
With config.DATA.VALIDATE_DEGRADE = (sigma1, sigma2, theta_deg, noise) (or degrade=(...), or --degrade s1,s2,theta,noise) the
generator's input is device_data.degrade(gt) with these fixed blur and noise parameters (key = the image's index) instead of the LR
file: the test set under the degradation DATA.DEGRADE trains on.  Either validation path, with or without VALIDATE_TILE; the printed
line and _metrics.txt name the parameters.
With config.DATA.VALIDATE_DEGRADE_JPEG = Q (or degrade_jpeg=Q, or --degrade-jpeg Q; 1..100) that input also goes through the JPEG
stage (device_data.jpeg, chroma DATA.DEGRADE_JPEG_CHROMA) at quality Q; without VALIDATE_DEGRADE the input is then the JPEG round trip
of the plain bicubic LR made from gt.  The printed line and _metrics.txt name the quality.
With config.DATA.VALIDATE_DEGRADE_SINC = omega (or degrade_sinc=omega, or --degrade-sinc OMEGA; 0 < omega <= pi) that input also goes
through the sinc low-pass filter of the second-order degradation (device_data.filter2d with kernels.sinc at this cutoff, window
DATA.DEGRADE2_KSIZE): after degrade(gt), or the plain bicubic LR made from gt, and before the JPEG stage.  The head line names it.
With config.DATA.VALIDATE_DEGRADE_RESIZE = s (or degrade_resize=s, or --degrade-resize S; 0.25 <= s <= 2) that input also goes through
the resize round trip of the second-order degradation (device_data.rescale: bicubic to the scale s and bicubic back, no noise): after
degrade(gt), or the plain bicubic LR made from gt, and before the sinc stage.  The head line names it.
With config.DATA.VALIDATE_DEGRADE_RESIZE1 = (s, m1, m2) (or degrade_resize1=(...), or --degrade-resize1 S[,M1,M2]; 0.125 <= s <= 2) that
input is made through the first stage's random resize (device_data.blur, then device_data.rescale_to): the blur of VALIDATE_DEGRADE,
gt to the scale s with the mode m1, the noise there, to the LR size with m2 - in the antialiased bicubic's place, before every other
stage.  The head line names it."""
from __future__ import annotations

import argparse
import os
from statistics import NormalDist

import numpy as np
import torch
from torch.utils.data import DataLoader

from .bicubic import Bicubic, NearestNeighbourUpscale
from .config import Config
from .dataset import TestImageDataset
from .model import Generator
from .st import st_distance
from .utils import PSNR, SSIM, bgr2ycbcr, load_state_dict, tensor2img


def confidence_interval(data, confidence=0.95):
    if len(data) < 2:
        return 0.0
    dist = NormalDist.from_samples(data)
    z = NormalDist().inv_cdf((1 + confidence) / 2.0)
    return dist.stdev * z / ((len(data) - 1) ** 0.5)


def image_metrics(sr: torch.Tensor, hr: torch.Tensor):
    """(psnr, ssim) of one SR/HR pair exactly as validate.py:79-99."""
    output = tensor2img(sr).astype(np.float32) / 255.0
    gt = tensor2img(hr).astype(np.float32) / 255.0
    output = bgr2ycbcr(output, only_y=True)
    gt = bgr2ycbcr(gt, only_y=True)
    return PSNR(output * 255, gt * 255), SSIM(output * 255, gt * 255)


def _save_png(path, bgr_u8):
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(bgr_u8[..., ::-1])).save(path)


def _st_params(config):
    """(sigma, rho, normalize) of the configured ``ST`` criterion, else StructureTensorLoss's defaults."""
    crit = config.MODEL.G_LOSS.CRITERIONS.get("ST")
    if crit is None:
        return 0.5, 2.0, True
    return float(crit.sigma), float(crit.rho), bool(crit.normalize)


def _lr_scale(output, lr_img):
    """The integer factor between a generator's output and its LR input."""
    return int(round(output.shape[2] / lr_img.shape[2]))


def _degrade_params(config, degrade):
    """None, or (sigma1, sigma2, theta_deg, noise) as four floats: the argument, else config.DATA.VALIDATE_DEGRADE."""
    if degrade is None:
        degrade = config.DATA.get("VALIDATE_DEGRADE", None)
    if not degrade:
        return None
    degrade = tuple(float(v) for v in degrade)
    if len(degrade) != 4:
        raise ValueError(f"VALIDATE_DEGRADE: expected (sigma1, sigma2, theta_deg, noise), got {degrade}")
    return degrade


def _jpeg_param(config, degrade_jpeg):
    """None, or the JPEG quality as an int in 1..100: the argument, else config.DATA.VALIDATE_DEGRADE_JPEG."""
    if degrade_jpeg is None:
        degrade_jpeg = config.DATA.get("VALIDATE_DEGRADE_JPEG", None)
    if degrade_jpeg is None:
        return None
    if int(degrade_jpeg) != degrade_jpeg or not 1 <= degrade_jpeg <= 100:
        raise ValueError(f"VALIDATE_DEGRADE_JPEG: expected a quality in 1..100, got {degrade_jpeg!r}")
    return int(degrade_jpeg)


def _sinc_param(config, degrade_sinc):
    """None, or the sinc filter's cutoff as a float in (0, pi]: the argument, else config.DATA.VALIDATE_DEGRADE_SINC."""
    if degrade_sinc is None:
        degrade_sinc = config.DATA.get("VALIDATE_DEGRADE_SINC", None)
    if degrade_sinc is None:
        return None
    if not 0 < float(degrade_sinc) <= np.pi:
        raise ValueError(f"VALIDATE_DEGRADE_SINC: expected a cutoff in (0, pi], got {degrade_sinc!r}")
    return float(degrade_sinc)


def _resize_param(config, degrade_resize):
    """None, or the resize round trip's scale as a float in [0.25, 2]: the argument, else config.DATA.VALIDATE_DEGRADE_RESIZE."""
    if degrade_resize is None:
        degrade_resize = config.DATA.get("VALIDATE_DEGRADE_RESIZE", None)
    if degrade_resize is None:
        return None
    if not 0.25 <= float(degrade_resize) <= 2:
        raise ValueError(f"VALIDATE_DEGRADE_RESIZE: expected a scale in [0.25, 2], got {degrade_resize!r}")
    return float(degrade_resize)


def _resize1_param(config, degrade_resize1):
    """None, or the first stage's resize as (s, m1, m2), s a float in [0.125, 2] and the modes names of device_data.RESIZE_MODES
    (a bare s, or (s,): bicubic both ways): the argument, else config.DATA.VALIDATE_DEGRADE_RESIZE1."""
    from .device_data import RESIZE_MODES
    if degrade_resize1 is None:
        degrade_resize1 = config.DATA.get("VALIDATE_DEGRADE_RESIZE1", None)
    if degrade_resize1 is None:
        return None
    v = tuple(degrade_resize1) if isinstance(degrade_resize1, (tuple, list)) else (degrade_resize1,)
    v = v + ("bicubic", "bicubic") if len(v) == 1 else v
    try:
        ok = len(v) == 3 and 0.125 <= float(v[0]) <= 2 and v[1] in RESIZE_MODES and v[2] in RESIZE_MODES
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"VALIDATE_DEGRADE_RESIZE1: expected (s, m1, m2), s in [0.125, 2], the modes of {tuple(RESIZE_MODES)}, got "
                         f"{degrade_resize1!r}")
    return float(v[0]), v[1], v[2]


_sinc_banks = {}


def _round_trip(lr, s):
    """lr [1,3,h,w] through device_data.rescale at the scale s: bicubic to (max(int(h s), ceil(h / 4)), the same for w), bicubic
    back, no noise; clamped and on the 1/255 grid."""
    from .device_data import rescale, rescale_rows, resize_size
    h, w = lr.shape[2:]
    rows = rescale_rows([(resize_size(h, s), resize_size(w, s))], ("bicubic", "bicubic"), 0.0, 0.0, 0, [(0, 0)])
    return rescale(lr, torch.from_numpy(rows))


def _degraded_input(hr_img, idx, config, degrade, jpeg=None, sinc=None, resize=None, resize1=None):
    """The generator's input under VALIDATE_DEGRADE / VALIDATE_DEGRADE_RESIZE1 / VALIDATE_DEGRADE_RESIZE / VALIDATE_DEGRADE_SINC /
    VALIDATE_DEGRADE_JPEG: degrade(hr) with the fixed parameters and key = the image's index (without VALIDATE_DEGRADE: neither blur
    nor noise, the plain bicubic's bits) - with resize1 = (s, m1, m2) the stage with its resize instead (degrade(resize_rows=): the
    blur, hr to the scale s with m1, the noise there, to the LR size with m2) - then the resize round trip at scale resize (bicubic
    both ways, no noise), then the sinc filter at cutoff sinc, then the JPEG stage at quality jpeg."""
    from .device_data import Degradation
    from .device_data import degrade as degrade_op
    ksize = int(config.DATA.get("DEGRADE_BLUR_KSIZE", 21))
    chroma = config.DATA.get("DEGRADE_JPEG_CHROMA", "420")
    if resize1:
        deg = Degradation.fixed(*(degrade or (0.0, 0.0, 0.0, 0.0)), key=idx, ksize=ksize, jpeg=jpeg or 0, jpeg_chroma=chroma,
                                resize=resize1)
        rows = deg.draw(1)
        first = deg.draw_resize(1, hr_img.shape[2], hr_img.shape[3], deg_rows=rows).to(hr_img.device)
        rows = rows.to(hr_img.device)
        if not (sinc or resize):
            return degrade_op(hr_img.to(torch.float32), rows, int(config.DATA.UPSCALE_FACTOR), ksize,
                              jpeg_chroma=chroma if jpeg else None, resize_rows=first)
    if sinc or resize:
        from . import kernels
        from .device_data import filter2d, filter_rows
        from .device_data import jpeg as jpeg_op
        k2 = int(config.DATA.get("DEGRADE2_KSIZE", 21))
        if not resize1:
            deg = Degradation.fixed(*(degrade or (0.0, 0.0, 0.0, 0.0)), key=idx, ksize=ksize, jpeg=jpeg or 0, jpeg_chroma=chroma)
            rows, first = deg.draw(1).to(hr_img.device), None
        lr = degrade_op(hr_img.to(torch.float32), rows, int(config.DATA.UPSCALE_FACTOR), ksize, resize_rows=first)
        if resize:
            lr = _round_trip(lr, resize)
        if sinc:
            key = (str(hr_img.device), k2, sinc)
            if key not in _sinc_banks:                       # the table and its one row: made once per (device, window, cutoff)
                _sinc_banks[key] = (torch.from_numpy(kernels.bank([kernels.sinc(k2, sinc)])).to(hr_img.device),
                                    torch.from_numpy(filter_rows([0], 0.0, 0.0, 0, [(0, 0)])).to(hr_img.device))
            bank, flt = _sinc_banks[key]
            lr = filter2d(lr, flt, bank)
        return jpeg_op(lr, rows, chroma, out=lr) if jpeg else lr
    deg = Degradation.fixed(*(degrade or (0.0, 0.0, 0.0, 0.0)), key=idx, ksize=ksize, jpeg=jpeg or 0, jpeg_chroma=chroma)
    return degrade_op(hr_img.to(torch.float32), deg.draw(1).to(hr_img.device), int(config.DATA.UPSCALE_FACTOR), ksize,
                      jpeg_chroma=chroma if jpeg else None)


def _metrics_on_device(generator, val_loader, config, save_images, concat_with_gt, st_params=None, with_lr=False, degrade=None,
                       jpeg=None, sinc=None, resize=None, resize1=None):
    """The per-image loop of _validate with everything on the device: generator forward -> sst_image_metrics into row idx of one
    [N,2] result buffer, ONE device-to-host copy after the loop.  Nothing syncs per image unless save_images is set (the uint8
    images tensor2img would make then cross per image and are written by _save_png).  st_params: also st_distance(output, hr) per
    image into an [N] buffer that crosses once as well -> third list; with_lr: the same for lr_consistency(output, lr) -> fourth list
    (LR-PSNR)."""
    from .metrics import image_metrics_device, lr_consistency, lr_psnr_from_mse, psnr_from_mse
    results = torch.empty(len(val_loader), 2, dtype=torch.float64, device=config.DEVICE)
    st_results = torch.empty(len(val_loader), dtype=torch.float64, device=config.DEVICE) if st_params else None
    lr_results = torch.empty(len(val_loader), dtype=torch.float64, device=config.DEVICE) if with_lr else None
    with torch.no_grad():
        for idx, (hr_img, lr_img) in enumerate(val_loader):
            lr_img = lr_img.to(config.DEVICE, non_blocking=True)
            hr_img = hr_img.to(config.DEVICE, non_blocking=True)
            if degrade or jpeg or sinc or resize or resize1:
                lr_img = _degraded_input(hr_img, idx, config, degrade, jpeg, sinc, resize, resize1)
            output = generator(lr_img)
            row = results[idx:idx + 1]
            if save_images:
                path = os.path.join(config.DATA.TEST_SR_IMAGES_DIR, config.EXP.NAME)
                os.makedirs(path, exist_ok=True)
                _, o, g = image_metrics_device(output, hr_img, want_u8=True, out=row)
                o = o[0].cpu().numpy()
                _save_png(f"{path}/{idx}.png", np.concatenate([o, g[0].cpu().numpy()], axis=1) if concat_with_gt else o)
            else:
                image_metrics_device(output, hr_img, out=row)
            if st_params:
                st_results[idx:idx + 1].copy_(st_distance(output, hr_img, *st_params))
            if with_lr:
                lr_results[idx:idx + 1].copy_(lr_consistency(output, lr_img, _lr_scale(output, lr_img)))
    host = results.cpu().tolist()
    all_lr = [lr_psnr_from_mse(m) for m in lr_results.cpu().tolist()] if with_lr else []
    return [psnr_from_mse(mse) for mse, _ in host], [ssim for _, ssim in host], st_results.cpu().tolist() if st_params else [], all_lr


def _validate(generator, val_loader, config, save_images=False, concat_with_gt=False, save_metrics=False, on_device=None,
              with_st=None, tile=None, with_lr=None, degrade=None, degrade_jpeg=None, degrade_sinc=None, degrade_resize=None,
              degrade_resize1=None):
    """degrade: None = config.DATA.VALIDATE_DEGRADE; (sigma1, sigma2, theta_deg, noise) = the generator's input is degrade(hr)
    (_degraded_input) instead of the loader's LR image, and the printed line and _metrics.txt start by saying so.
    degrade_jpeg: None = config.DATA.VALIDATE_DEGRADE_JPEG; Q in 1..100 = that input, or without `degrade` the plain bicubic LR made
    from hr, goes through the JPEG stage at quality Q, and the head line names it.
    degrade_sinc: None = config.DATA.VALIDATE_DEGRADE_SINC; omega in (0, pi] = that input goes through the sinc filter at this cutoff
    before the JPEG stage, and the head line names it.
    degrade_resize: None = config.DATA.VALIDATE_DEGRADE_RESIZE; s in [0.25, 2] = that input goes through the resize round trip at
    this scale (bicubic both ways, no noise) before the sinc filter, and the head line names it.
    degrade_resize1: None = config.DATA.VALIDATE_DEGRADE_RESIZE1; (s, m1, m2), s in [0.125, 2] = that input is made through the first
    stage's resize (the blur, hr to the scale s with m1, the noise there, to the LR size with m2) instead of the antialiased bicubic,
    before every other stage, and the head line names it.
    on_device: None = config.DATA.VALIDATE_ON_DEVICE; True = metrics by the HIP kernel, one host copy per pass
    (_metrics_on_device); False = the host loop below.  Same averages, same printed line, same _metrics.txt either way.
    with_st: None = config.DATA.VALIDATE_ST; True = every image also gets st.st_distance(output, hr) with the configured ``ST``
    criterion's (sigma, rho, normalize), _metrics.txt and the printed line gain an ``ST:`` column and the return value becomes
    (psnr, ssim, st); False = everything as without the option.
    with_lr: None = config.DATA.VALIDATE_LR; True = every image also gets metrics.lr_consistency(output, the loader's lr_img) as an
    ``LR-PSNR:`` column (after ``ST:`` when both are on) and the return value gains (lr_psnr,) at its end; False = as without it.
    tile: None = config.DATA.VALIDATE_TILE; T > 0 = a Generator runs through upscale.Upscaler(tile=T) with the exact halo (an image
    that fits in one window takes the plain forward, so small test sets give the numbers they give without the option); 0 = off."""
    if tile is None:
        tile = int(config.DATA.get("VALIDATE_TILE", 0))
    if tile and isinstance(generator, Generator):
        from .upscale import Upscaler
        generator = Upscaler(generator, tile=tile)
    if on_device is None:
        on_device = bool(config.DATA.get("VALIDATE_ON_DEVICE", False))
    if with_st is None:
        with_st = bool(config.DATA.get("VALIDATE_ST", False))
    st_params = _st_params(config) if with_st else None
    if with_lr is None:
        with_lr = bool(config.DATA.get("VALIDATE_LR", False))
    degrade = _degrade_params(config, degrade)
    jpeg = _jpeg_param(config, degrade_jpeg)
    sinc = _sinc_param(config, degrade_sinc)
    resize = _resize_param(config, degrade_resize)
    resize1 = _resize1_param(config, degrade_resize1)
    parts, made = [], "degrade(GT)" if degrade else ("GT" if resize1 else "bicubic(GT)")              # the head line: what made the input, then its parameters
    if degrade:
        parts.append("sigma {:g} / {:g}, theta {:g} deg, noise {:g}".format(*degrade))
    for on, name, part in ((resize1, "resize1", "first-stage resize at scale {:g} ({}, then {} to the LR size)".format(*resize1)
                            if resize1 else ""),
                           (resize, "resize", f"resize round trip at scale {resize:g} (bicubic)" if resize else ""),
                           (sinc, "sinc", f"sinc cutoff {sinc:g}" if sinc else ""),
                           (jpeg, "jpeg", f"JPEG quality {jpeg} ({config.DATA.get('DEGRADE_JPEG_CHROMA', '420')})" if jpeg else "")):
        if on:
            parts.append(part)
            made = made if degrade else f"{name}({made})"
    deg_head = f"LR = {made}: {', '.join(parts)} | " if parts else ""
    file = None
    if save_metrics:
        path = os.path.join(config.DATA.TEST_SR_IMAGES_DIR, config.EXP.NAME)
        os.makedirs(path, exist_ok=True)
        file = open(os.path.join(path, "_metrics.txt"), mode="w")
        if deg_head:
            file.write(deg_head + "\n")
    all_psnr, all_ssim, all_st, all_lr = [], [], [], []
    if on_device:
        all_psnr, all_ssim, all_st, all_lr = _metrics_on_device(generator, val_loader, config, save_images, concat_with_gt, st_params,
                                                                with_lr, degrade, jpeg, sinc, resize, resize1)
        if file:
            for idx, (psnr, ssim) in enumerate(zip(all_psnr, all_ssim)):
                st_col = f" | ST: {all_st[idx]:.4f}" if with_st else ""
                lr_col = f" | LR-PSNR: {all_lr[idx]:.2f}" if with_lr else ""
                file.write(f"{idx}.png | PSNR: {psnr:.2f} | SSIM: {ssim:.4f}{st_col}{lr_col}\n")
    else:
        with torch.no_grad():
            for idx, (hr_img, lr_img) in enumerate(val_loader):
                lr_img = lr_img.to(config.DEVICE)
                hr_img = hr_img.to(config.DEVICE)
                if degrade or jpeg or sinc or resize or resize1:
                    lr_img = _degraded_input(hr_img, idx, config, degrade, jpeg, sinc, resize, resize1)
                output = generator(lr_img)
                if save_images:
                    path = os.path.join(config.DATA.TEST_SR_IMAGES_DIR, config.EXP.NAME)
                    os.makedirs(path, exist_ok=True)
                    o, g = tensor2img(output), tensor2img(hr_img)
                    _save_png(f"{path}/{idx}.png", np.concatenate([o, g], axis=1) if concat_with_gt else o)
                psnr, ssim = image_metrics(output, hr_img)
                all_psnr.append(psnr)
                all_ssim.append(ssim)
                st_col = ""
                if with_st:                                   # the host-metric path syncs per image anyway
                    all_st.append(st_distance(output, hr_img, *st_params).item())
                    st_col = f" | ST: {all_st[-1]:.4f}"
                lr_col = ""
                if with_lr:
                    from .metrics import lr_consistency, lr_psnr_from_mse
                    all_lr.append(lr_psnr_from_mse(lr_consistency(output, lr_img, _lr_scale(output, lr_img)).item()))
                    lr_col = f" | LR-PSNR: {all_lr[-1]:.2f}"
                if file:
                    file.write(f"{idx}.png | PSNR: {psnr:.2f} | SSIM: {ssim:.4f}{st_col}{lr_col}\n")
    avg_psnr = sum(all_psnr) / len(all_psnr)
    avg_ssim = sum(all_ssim) / len(all_ssim)
    out = (f"[Test] | {deg_head}PSNR: {avg_psnr:.2f} ± {confidence_interval(all_psnr):.2f} | "
           f"SSIM: {avg_ssim:.4f} ± {confidence_interval(all_ssim):.4f} | ")
    if with_st:
        avg_st = sum(all_st) / len(all_st)
        out += f"ST: {avg_st:.4f} ± {confidence_interval(all_st):.4f} | "
    if with_lr:
        avg_lr = sum(all_lr) / len(all_lr)
        out += f"LR-PSNR: {avg_lr:.2f} ± {confidence_interval(all_lr):.2f} | "
    out += "\n"
    print(out)
    if file:
        file.write("\n" + out + "\n")
        file.close()
    return (avg_psnr, avg_ssim) + ((avg_st,) if with_st else ()) + ((avg_lr,) if with_lr else ())


def test(config: Config, save_images: bool = True, g_path: str = None, concat_w_gt: bool = False, dataset=None, on_device=None,
         with_st=None, tile=None, with_lr=None, degrade=None, degrade_jpeg=None, degrade_sinc=None, degrade_resize=None,
         degrade_resize1=None):
    if not g_path:                # the averaged generator's best when the run kept one (SOLVER.G_EMA_DECAY), else the last iterate's
        g_path = f"results/{config.EXP.NAME}/g_ema_best.pth"
        if not os.path.exists(g_path):
            g_path = f"results/{config.EXP.NAME}/g_best.pth"
    ds = dataset if dataset is not None else TestImageDataset(config.DATA.TEST_GT_IMAGES_DIR, config.DATA.TEST_LR_IMAGES_DIR)
    loader = DataLoader(ds, batch_size=1, shuffle=False, num_workers=0, drop_last=False)
    if config.EXP.NAME == "bicubic":
        generator = Bicubic(device=config.DEVICE).to(config.DEVICE)
    elif config.EXP.NAME == "nearest":
        generator = NearestNeighbourUpscale(config.DATA.UPSCALE_FACTOR).to(config.DEVICE)
    else:
        generator = Generator(config).to(config.DEVICE)
        generator = load_state_dict(generator, torch.load(g_path, map_location=config.DEVICE, weights_only=True))
        generator.eval()
    return _validate(generator, loader, config, save_images=save_images, concat_with_gt=concat_w_gt, save_metrics=True,
                     on_device=on_device, with_st=with_st, tile=tile, with_lr=with_lr, degrade=degrade, degrade_jpeg=degrade_jpeg,
                     degrade_sinc=degrade_sinc, degrade_resize=degrade_resize, degrade_resize1=degrade_resize1)


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--name", type=str, default=None)
    parser.add_argument("--g-path", type=str, default=None)
    parser.add_argument("--test-set", type=str, default=None)
    parser.add_argument("--no-images", action="store_true")
    parser.add_argument("--on-device", action="store_true", help="PSNR / SSIM by the HIP kernel (DATA.VALIDATE_ON_DEVICE)")
    parser.add_argument("--st", action="store_true", help="also the structure-tensor distance per image (DATA.VALIDATE_ST)")
    parser.add_argument("--tile", type=int, default=None, help="run the generator tiled, windows of this many LR pixels (DATA.VALIDATE_TILE)")
    parser.add_argument("--lr-consistency", action="store_true", help="also the LR-PSNR of the re-downscaled output per image (DATA.VALIDATE_LR)")
    parser.add_argument("--degrade", type=str, default=None, metavar="S1,S2,THETA,NOISE",
                        help="feed the generator degrade(gt) with this fixed blur and noise instead of the LR files (DATA.VALIDATE_DEGRADE)")
    parser.add_argument("--degrade-jpeg", type=int, default=None, metavar="Q",
                        help="also take that input (or, without --degrade, the bicubic LR made from gt) through the JPEG stage at "
                             "quality Q (DATA.VALIDATE_DEGRADE_JPEG)")
    parser.add_argument("--degrade-sinc", type=float, default=None, metavar="OMEGA",
                        help="also take that input through the sinc low-pass filter at cutoff OMEGA in (0, pi], before the JPEG stage "
                             "(DATA.VALIDATE_DEGRADE_SINC)")
    parser.add_argument("--degrade-resize", type=float, default=None, metavar="S",
                        help="also take that input through the resize round trip at scale S in [0.25, 2] (bicubic both ways, no noise), "
                             "before the sinc stage (DATA.VALIDATE_DEGRADE_RESIZE)")
    parser.add_argument("--degrade-resize1", type=str, default=None, metavar="S[,M1,M2]",
                        help="make that input through the first stage's random resize at scale S in [0.125, 2] of the HR size: mode M1 "
                             "there, M2 to the LR size (area | bilinear | bicubic; default bicubic), before every other stage "
                             "(DATA.VALIDATE_DEGRADE_RESIZE1)")
    a = parser.parse_args()
    cfg = Config()
    if a.name:
        cfg.EXP.NAME = a.name
    if a.test_set:
        cfg.DATA.TEST_SET = a.test_set
        cfg.DATA.TEST_GT_IMAGES_DIR = f"/work3/{cfg.EXP.USER}/data/{a.test_set}/GTmod12"
        cfg.DATA.TEST_LR_IMAGES_DIR = f"/work3/{cfg.EXP.USER}/data/{a.test_set}/LRbicx4"
    test(cfg, save_images=not a.no_images, g_path=a.g_path, on_device=True if a.on_device else None,
         with_st=True if a.st else None, tile=a.tile, with_lr=True if a.lr_consistency else None,
         degrade=tuple(float(v) for v in a.degrade.split(",")) if a.degrade else None, degrade_jpeg=a.degrade_jpeg,
         degrade_sinc=a.degrade_sinc, degrade_resize=a.degrade_resize,
         degrade_resize1=(lambda v: (float(v[0]),) + tuple(v[1:]))(a.degrade_resize1.split(",")) if a.degrade_resize1 else None)
