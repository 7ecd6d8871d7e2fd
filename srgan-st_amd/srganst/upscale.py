"""Upscale whole images: tiled generator inference with exact halos.

In eval mode (BatchNorm folded to an affine of the running statistics) the generator is a finite-support convolution stack, so a
window of the LR image with a large enough halo gives, inside the halo, exactly the whole-image result: no blending, no seams.
``receptive_radius`` is that halo, ``TilePlan`` cuts an image into equal-size windows that never leave it (each layer's zero padding
then falls on the image border exactly as in the whole-image forward) and gives every pixel to one window, ``Upscaler`` runs the
windows in batches through the HIP generator: one launch cuts (and, for the x8 self-ensemble, flips / transposes) a batch of
windows (csrc/tiles.hip: sst_tile_gather), one launch pastes the owned rectangles of the result into the output canvas
(sst_tile_scatter), one launch quantises the canvas to uint8 (sst_canvas_to_u8).  ``tiled_reference`` is the same procedure in plain
torch on any device and dtype: the restatement the tests compare against (test infrastructure; the product path is the kernels).

    python -m srganst.upscale --g-path G --in-dir D --out-dir O [--tile 256 --halo R --batch 8 --ensemble 1 --name NAME]
"""
from __future__ import annotations

import argparse
import math
import os
import time
from concurrent.futures import ThreadPoolExecutor
from fractions import Fraction

import numpy as np
import torch
from torch import Tensor

from . import _abi
from .device_data import decode_threads, dihedral, lut

ACT_LIMIT = 1 << 29          # elements: the pipelined conv entries take activations below this (32-bit byte offsets)


def receptive_radius(n_rcb: int, upscale: int) -> int:
    """LR pixels beyond which the eval-mode generator's output does not depend on its input: 4 (conv1, 9x9) + 2 per residual block
    + 1 (conv2) + 2^-k for the 3x3 conv of the k-th up-sampling block (it runs at 2^k times the LR resolution) + 4 / upscale
    (conv3, 9x9 at the output resolution), rounded up."""
    n_up = int(round(math.log2(upscale)))
    if n_rcb < 0 or 2 ** n_up != upscale:
        raise ValueError(f"receptive_radius: n_rcb {n_rcb} / upscale {upscale} (a power of two) out of range")
    r = Fraction(4 + 2 * n_rcb + 1) + sum(Fraction(1, 2 ** k) for k in range(n_up)) + Fraction(4, upscale)
    return math.ceil(r)


def inverse_dihedral(t: int) -> int:
    """The element that undoes device_data.dihedral's t (= 4*transpose + 2*vflip + 1*hflip, applied in that order):
    dihedral(dihedral(x, t), inverse_dihedral(t)) == x, on rectangles too.  The flips are their own inverses; behind a transpose the
    two flips change places."""
    return t if t < 4 else 4 | ((t & 1) << 1) | ((t & 2) >> 1)


def _axis(L: int, tile: int, halo: int):
    """Windows of one axis of length L: (window side t, [(start, owned from, owned to)])."""
    t = min(tile, L)
    if t == L:
        return t, [(0, 0, L)]
    S = t - 2 * halo
    if S <= 0:
        raise ValueError(f"TilePlan: tile {tile} leaves no stride beside two halos of {halo} (tile must exceed 2 * halo = {2 * halo})")
    n = -(-(L - t) // S) + 1
    out, end = [], 0
    for k in range(n):
        s = min(k * S, L - t)
        own1 = L if k == n - 1 else s + t - halo
        out.append((s, end, own1))
        end = own1
    return t, out


class TilePlan:
    """Windows of an H x W image for tiles of at most `tile` pixels a side with `halo` pixels of context: per axis of length L the
    window side is t = min(tile, L) (all windows of an image have one shape th x tw), the stride t - 2*halo, the last window moved
    back to end at L; window k owns from the end of window k-1's range to `halo` before its own end (the first from 0, the last up
    to L), so owned ranges partition the axis and every owned pixel is at least `halo` from each window edge inside the image.
    rows: int32 [n, 6] = (y0, x0, oy0, oy1, ox0, ox1) in LR pixels, the row-major product of the two axes."""

    def __init__(self, H: int, W: int, tile: int, halo: int):
        if H <= 0 or W <= 0 or tile <= 0 or halo < 0:
            raise ValueError(f"TilePlan: bad argument (H {H}, W {W}, tile {tile}, halo {halo})")
        self.H, self.W, self.tile, self.halo = int(H), int(W), int(tile), int(halo)
        self.th, ys = _axis(self.H, self.tile, self.halo)
        self.tw, xs = _axis(self.W, self.tile, self.halo)
        self.ny, self.nx = len(ys), len(xs)
        self.rows = np.array([(y0, x0, a0, a1, b0, b1) for y0, a0, a1 in ys for x0, b0, b1 in xs], np.int32).reshape(-1, 6)

    def __len__(self) -> int:
        return len(self.rows)


def tiled_reference(forward, x: Tensor, plan: TilePlan, upscale: int, ensemble: int = 1) -> Tensor:
    """What Upscaler computes, in plain torch: x [1,3,H,W] -> [1,3,s*H,s*W].  The windows of `plan` are cut from x and stacked,
    `forward` runs on the stack, the owned rectangles of its result are pasted into the output.  ensemble=8: the mean over the eight
    dihedral elements t of dihedral(forward(dihedral(stack, t)), inverse_dihedral(t)) (summed in the order of t, then / 8)."""
    if ensemble not in (1, 8):
        raise ValueError("tiled_reference: ensemble must be 1 or 8")
    s, th, tw = int(upscale), plan.th, plan.tw
    rows = plan.rows.tolist()
    stack = torch.stack([x[0, :, y0:y0 + th, x0:x0 + tw] for y0, x0, *_ in rows])
    total = None
    for t in range(ensemble):
        sr = dihedral(forward(dihedral(stack, t).contiguous()), inverse_dihedral(t))
        total = sr if total is None else total + sr
    if ensemble > 1:
        total = total / ensemble
    out = x.new_empty(1, x.shape[1], s * plan.H, s * plan.W)
    for b, (y0, x0, oy0, oy1, ox0, ox1) in enumerate(rows):
        out[0, :, s * oy0:s * oy1, s * ox0:s * ox1] = total[b, :, s * (oy0 - y0):s * (oy1 - y0), s * (ox0 - x0):s * (ox1 - x0)]
    return out


def _pad16(n: int) -> int:
    return (n + 15) & ~15


# ---------------------------------------------------------------------------------------------------- the three launches
def tile_gather(src: Tensor, H: int, W: int, desc: Tensor, th: int, tw: int, t: int, lut_dev: Tensor | None = None) -> Tensor:
    """src: flat uint8 (HWC/RGB image at its start, numel a multiple of 16) or fp32 [3,H,W]; desc int32 [B,3] = (y0, x0, t) on the
    device -> fp32 [B,3,th',tw'] (sst_tile_gather)."""
    B = desc.shape[0]
    if desc.dtype != torch.int32 or desc.dim() != 2 or desc.shape[1] != 3 or not desc.is_contiguous():
        raise _abi.HipPathError("tile_gather: desc must be a contiguous int32 [B, 3] tensor")
    Ho, Wo = (tw, th) if t & 4 else (th, tw)
    u8 = src.dtype == torch.uint8
    if not u8 and (src.dtype != torch.float32 or tuple(src.shape) != (3, H, W)):
        raise _abi.HipPathError(f"tile_gather: the source must be flat uint8 or fp32 [3, {H}, {W}], got {src.dtype} {tuple(src.shape)}")
    with torch.cuda.device(src.device):
        out = torch.empty(B, 3, Ho, Wo, dtype=torch.float32, device=src.device)
        _abi.check(_abi.lib().sst_tile_gather(_abi.ptr(src) if u8 else None, None if u8 else _abi.ptr(src), src.numel() * src.element_size(),
                                              H, W, _abi.ptr(desc), B, th, tw, t, _abi.ptr(lut_dev) if u8 else None, _abi.ptr(out),
                                              _abi.stream_ptr()), "sst_tile_gather")
    return out


def tile_scatter(tiles: Tensor, rows: Tensor, H: int, W: int, th: int, tw: int, scale: int, t: int, canvas: Tensor,
                 accumulate: bool = False) -> Tensor:
    """tiles fp32 [B,3,s*th',s*tw'], rows int32 [B,6] on the device -> the owned rectangles into canvas fp32 [3,s*H,s*W]
    (sst_tile_scatter)."""
    B = rows.shape[0]
    Ho, Wo = (tw, th) if t & 4 else (th, tw)
    if rows.dtype != torch.int32 or rows.dim() != 2 or rows.shape[1] != 6 or not rows.is_contiguous():
        raise _abi.HipPathError("tile_scatter: rows must be a contiguous int32 [B, 6] tensor")
    if tiles.dtype != torch.float32 or tuple(tiles.shape) != (B, 3, scale * Ho, scale * Wo):
        raise _abi.HipPathError(f"tile_scatter: tiles must be fp32 {(B, 3, scale * Ho, scale * Wo)}, got {tuple(tiles.shape)}")
    if canvas.dtype != torch.float32 or tuple(canvas.shape) != (3, scale * H, scale * W):
        raise _abi.HipPathError(f"tile_scatter: the canvas must be fp32 {(3, scale * H, scale * W)}, got {tuple(canvas.shape)}")
    with torch.cuda.device(canvas.device):
        _abi.check(_abi.lib().sst_tile_scatter(_abi.ptr(tiles), _abi.ptr(rows), B, H, W, th, tw, scale, t, _abi.ptr(canvas),
                                               int(bool(accumulate)), _abi.stream_ptr()), "sst_tile_scatter")
    return canvas


def canvas_to_u8(canvas: Tensor, scale: float = 1.0) -> Tensor:
    """canvas fp32 [3,H,W] -> uint8 [H,W,3] RGB, tensor2img's quantisation of canvas * scale (sst_canvas_to_u8)."""
    if canvas.dtype != torch.float32 or canvas.dim() != 3 or canvas.shape[0] != 3:
        raise _abi.HipPathError(f"canvas_to_u8: the canvas must be fp32 [3, H, W], got {canvas.dtype} {tuple(canvas.shape)}")
    _, H, W = canvas.shape
    with torch.cuda.device(canvas.device):
        out = torch.empty(H, W, 3, dtype=torch.uint8, device=canvas.device)
        _abi.check(_abi.lib().sst_canvas_to_u8(_abi.ptr(canvas), H, W, float(scale), _abi.ptr(out), _abi.stream_ptr()), "sst_canvas_to_u8")
    return out


# ---------------------------------------------------------------------------------------------------- Upscaler
class Upscaler:
    """A trained generator applied to whole images of any size.  tile: window side in LR pixels; halo: None = receptive_radius of the
    generator, which makes the result the whole-image forward's (up to fp32 summation order inside the conv kernels); a smaller
    halo costs less - the work overhead is (tile / (tile - 2*halo))^2 - and is APPROXIMATE: seams of the size the missing context
    causes.  batch: windows per generator call, capped so that the largest activation of a call stays below 2^29 elements (the
    pipelined conv kernels' limit).  ensemble: 1, or 8 = the mean over the eight flips / transpositions of every window.
    An image that fits in one window runs as the plain B = 1 forward."""

    def __init__(self, generator, tile: int = 256, halo: int | None = None, batch: int = 8, ensemble: int = 1):
        if generator.training:
            raise ValueError("Upscaler: the generator must be in eval() mode (train-mode BatchNorm statistics depend on the batch: "
                             "tiles would not reproduce the whole image)")
        if ensemble not in (1, 8):
            raise ValueError(f"Upscaler: ensemble must be 1 or 8, got {ensemble}")
        if tile <= 0 or batch <= 0:
            raise ValueError(f"Upscaler: tile {tile} and batch {batch} must be positive")
        self.generator = generator
        self.n_rcb, self.scale = len(generator.trunk), 2 ** len(generator.upsampling)
        self.channels = generator.conv1[0].out_channels
        self.tile, self.batch, self.ensemble = int(tile), int(batch), int(ensemble)
        self.halo = receptive_radius(self.n_rcb, self.scale) if halo is None else int(halo)
        if self.halo < 0:
            raise ValueError(f"Upscaler: halo {halo} must not be negative")
        self.device = next(generator.parameters()).device
        self._lut = None

    def plan(self, H: int, W: int) -> TilePlan:
        return TilePlan(H, W, self.tile, self.halo)

    def batch_for(self, th: int, tw: int) -> int:
        """Windows per generator call: `batch`, capped by the activation limit B * (s*th) * (s*tw) * C / 4 < 2^29 (the input of the
        last up-sampling conv, the largest NHWC tensor of the forward)."""
        per = self.scale * th * self.scale * tw * self.channels // 4
        cap = (ACT_LIMIT - 1) // max(per, 1)
        if cap < 1:
            raise ValueError(f"Upscaler: one {tw}x{th} window already has an activation of {per} elements (limit 2^29); use a smaller tile")
        return min(self.batch, cap)

    def _canvas(self, src: Tensor, H: int, W: int) -> Tensor:
        """src: padded flat uint8 HWC image or fp32 [3,H,W] on the device -> the fp32 canvas [3,sH,sW]: the SUM over the ensemble's
        passes (the caller scales by 1 / ensemble)."""
        plan = self.plan(H, W)
        s, th, tw = self.scale, plan.th, plan.tw
        B = self.batch_for(th, tw)
        rows = torch.from_numpy(plan.rows).to(self.device)
        if src.dtype == torch.uint8 and self._lut is None:
            self._lut = lut(self.device)
        canvas = torch.empty(3, s * H, s * W, dtype=torch.float32, device=self.device)      # every pixel is owned by one window
        with torch.no_grad():
            for t in range(self.ensemble):
                desc = torch.cat([rows[:, :2], torch.full_like(rows[:, :1], t)], dim=1).contiguous()
                for i in range(0, len(plan), B):
                    lr = tile_gather(src, H, W, desc[i:i + B], th, tw, t, self._lut)
                    sr = self.generator(lr)
                    tile_scatter(sr, rows[i:i + B], H, W, th, tw, s, t, canvas, accumulate=t > 0)
        return canvas

    def __call__(self, lr: Tensor) -> Tensor:
        """lr fp32 [1,3,H,W] on the generator's device -> fp32 [1,3,sH,sW] in [0,1]: a drop-in for the generator."""
        if lr.dim() != 4 or lr.shape[0] != 1 or lr.shape[1] != 3 or lr.dtype != torch.float32:
            raise _abi.HipPathError(f"Upscaler: expected one fp32 image [1, 3, H, W], got {lr.dtype} {tuple(lr.shape)}")
        _, _, H, W = lr.shape
        if self.ensemble == 1 and H <= self.tile and W <= self.tile:
            with torch.no_grad():
                return self.generator(lr)
        canvas = self._canvas(lr[0].contiguous(), H, W)
        if self.ensemble > 1:
            canvas.mul_(1.0 / self.ensemble)          # a power of two: the mean, exactly
        return canvas.unsqueeze(0)

    def upscale_u8(self, img) -> Tensor:
        """img: uint8 [H,W,3] RGB (numpy array or tensor, as dataset.read_image_hwc decodes it) -> uint8 [sH,sW,3] RGB on the
        generator's device."""
        if isinstance(img, np.ndarray):          # PIL hands out read-only arrays; torch wants a writable one
            img = np.ascontiguousarray(img) if img.flags.writeable else img.copy()
        img = torch.as_tensor(img)
        if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
            raise _abi.HipPathError(f"Upscaler.upscale_u8: expected uint8 [H, W, 3], got {img.dtype} {tuple(img.shape)}")
        H, W, _ = img.shape
        n = H * W * 3
        buf = torch.zeros(_pad16(n), dtype=torch.uint8, device=self.device)      # the gather's contract: padded to 16 bytes
        buf[:n].copy_(img.reshape(-1), non_blocking=True)
        canvas = self._canvas(buf, H, W)
        return canvas_to_u8(canvas, 1.0 / self.ensemble)


# ---------------------------------------------------------------------------------------------------- command line
def generator_from_checkpoint(g_path: str, device):
    """The generator a checkpoint was trained as: width, depth and scale are read from its tensors."""
    from .config import Config
    from .model import Generator
    from .utils import load_state_dict
    sd = torch.load(g_path, map_location=device, weights_only=True)
    keys = [k[10:] if k.startswith("_orig_mod.") else k for k in sd]
    cfg = Config()
    cfg.MODEL.G_N_CHANNEL = next(v for k, v in sd.items() if k.endswith("conv1.0.weight")).shape[0]
    cfg.MODEL.G_N_RCB = 1 + max((int(k.split(".")[1]) for k in keys if k.startswith("trunk.")), default=-1)
    cfg.DATA.UPSCALE_FACTOR = 2 ** (1 + max((int(k.split(".")[1]) for k in keys if k.startswith("upsampling.")), default=-1))
    g = load_state_dict(Generator(cfg).to(device), sd)
    return g.eval()


def upscale_dir(up: Upscaler, in_dir: str, out_dir: str) -> tuple[int, float]:
    """Every image of in_dir -> out_dir/<same name, .png>.  Decode and encode on a thread pool, the device work on this thread.
    -> (images, seconds)."""
    from PIL import Image
    from .dataset import read_image_hwc
    names = sorted(n for n in os.listdir(in_dir) if not n.startswith(".") and os.path.isfile(os.path.join(in_dir, n)))
    if not names:
        raise ValueError(f"upscale: no images under {in_dir}")
    os.makedirs(out_dir, exist_ok=True)

    def save(name, arr):
        Image.fromarray(arr).save(os.path.join(out_dir, os.path.splitext(name)[0] + ".png"))

    t0 = time.perf_counter()
    with ThreadPoolExecutor(decode_threads()) as pool:
        decoded = [pool.submit(read_image_hwc, os.path.join(in_dir, n)) for n in names]
        writes = []
        for name, fut in zip(names, decoded):
            sr = up.upscale_u8(fut.result())
            writes.append(pool.submit(save, name, sr.cpu().numpy()))
        for w in writes:
            w.result()
    return len(names), time.perf_counter() - t0


def main(argv=None) -> None:
    p = argparse.ArgumentParser(description="Upscale every image of a directory with a trained generator (tiled, exact halos).")
    p.add_argument("--g-path", type=str, default=None, help="generator checkpoint (default results/<name>/g_best.pth)")
    p.add_argument("--name", type=str, default="experiment-name")
    p.add_argument("--in-dir", type=str, required=True)
    p.add_argument("--out-dir", type=str, required=True)
    p.add_argument("--tile", type=int, default=256, help="window side in LR pixels")
    p.add_argument("--halo", type=int, default=None, help="context per window side; default: the receptive radius (exact)")
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--ensemble", type=int, default=1, choices=(1, 8))
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise _abi.HipPathError("upscale: needs a ROCm device (there is no CPU fallback)")
    g = generator_from_checkpoint(a.g_path or f"results/{a.name}/g_best.pth", "cuda:0")
    up = Upscaler(g, tile=a.tile, halo=a.halo, batch=a.batch, ensemble=a.ensemble)
    n, dt = upscale_dir(up, a.in_dir, a.out_dir)
    print(f"[Upscale] {n} images in {dt:.2f} s | {n / dt:.3f} images/s | tile {up.tile} halo {up.halo} batch {up.batch} "
          f"ensemble {up.ensemble}")


if __name__ == "__main__":
    main()
