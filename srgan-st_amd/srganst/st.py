"""Structure-tensor maps on the HIP path (csrc/st_maps.hip: sst_st_maps): the fields the structure-tensor loss integrates.

What the reference studies in its visualization/ and data-exploration/ notebooks with utils.structure_tensor and
utils.compute_distance (utils.py:212-280), from the arithmetic of the loss kernels themselves (csrc/st_tile.h): the tensor field
(Jxx, Jyy, Jxy) of an image, its trace / orientation / coherence, the per-pixel Riemannian distance d between an SR image and its
ground truth (the loss's integrand), and the per-image mean of d - the quantity a run with the ``ST`` criterion optimises,
reported per test image by validate.py when DATA.VALIDATE_ST is set.

These are ANALYSIS ops, not criteria: they run under no_grad semantics (inputs are detached, nothing here is differentiable).
Train with srganst.loss.StructureTensorLoss.

Axis convention - the reference's names, not intuition: utils.py:219 reshapes the derivative taps of Ix to (1,1,-1,1), so "x" is the
HEIGHT axis (dim -2) and "y" the width axis.  Plane 0 (Jxx) carries the energy of an image that varies only from row to row.  In the
double-angle features (t, c2, s2):
  an image varying only along W gives c2 = -1,   an image varying only along H gives c2 = +1,
  sin(0.5 (col + row)) gives s2 = +1,            sin(0.5 (col - row)) gives s2 = -1.
"""
from __future__ import annotations

import torch
from torch import Tensor

from . import _abi
from ._abi import HipPathError
from .loss import _workspace, st_route

OUTPUTS = ("Sx", "Sgt", "Fx", "Fgt", "d", "tile_sums", "distance")
_NEED_GT = ("Sgt", "Fgt", "d", "tile_sums", "distance")


def workspace_floats(B: int, H: int, W: int) -> int:
    """Number of 32 x 32 tiles of a [B,3,H,W] batch = floats of ``tile_sums``."""
    return _workspace("st_maps", B, H, W, n=1)[0]


def general_scratch_floats(B: int, H: int, W: int) -> int:
    """Floats of the plane workspace of the general path (csrc/st_general.hip: sst_st_general_maps) = 14 B H W."""
    return _workspace("st_general", B, H, W, n=3)[0]


def _checked(name: str, t) -> Tensor:
    if not isinstance(t, Tensor) or not t.is_cuda:
        raise HipPathError(f"st_maps: {name} must be a tensor on a ROCm device (no CPU fallback)")
    if t.dtype != torch.float32:
        raise HipPathError(f"st_maps: {name} must be fp32, got {t.dtype}")
    if t.dim() != 4 or t.shape[1] != 3 or min(t.shape) < 1:
        raise HipPathError(f"st_maps: {name} must be [B,3,H,W], got {tuple(t.shape)}")
    return t.detach().contiguous()


def st_maps(sr: Tensor, gt: Tensor | None = None, sigma: float = 0.5, rho: float = 2.0, normalize: bool = True,
            want=("Sx", "d")) -> dict:
    """The general form: sst_st_maps (one launch) or, off the two built radius pairs, sst_st_general_maps -> dict of the outputs
    named in ``want``.

    sr, gt: fp32 [B,3,H,W] on one ROCm device (made contiguous if they are not); gt may be None when only maps of sr are wanted.
    want, any of:
      "Sx", "Sgt"   [B,3,H,W]  (Jxx, Jyy, Jxy) of sr / gt, the loss's plane order ("x" = the height axis, see the module docstring)
      "Fx", "Fgt"   [B,3,H,W]  (t, c2, s2): t = Jxx + Jyy, c2 = (Jxx - Jyy) / (t + 1e-12), s2 = 2 Jxy / (t + 1e-12)
      "d"           [B,H,W]    per-pixel distance between the structure tensors of sr and gt (StructureTensorLoss's integrand)
      "tile_sums"   [B,tiles]  fp32 sum of d over each 32 x 32 tile
      "distance"    [B] fp64   per-image mean of d: the tile sums added in fp64 in index order, over H * W
    (sigma, rho): any pair whose radii max(int(4 s + 0.5), 1) are at most 8 (sigma) and 20 (rho), as for StructureTensorLoss and by
    the same routes: radii (2, 8) and (4, 10) run the tile kernel, every other pair the separable passes of csrc/st_general.hip (in a
    workspace of 14 B H W floats allocated per call); beyond the bound HipPathError.  Analysis op: inputs are detached, no gradient.
    Runs on the current stream, never syncs with the host, bit-identical from call to call."""
    want = tuple(want)
    unknown = [w for w in want if w not in OUTPUTS]
    if unknown or not want:
        raise HipPathError(f"st_maps: want must name at least one of {OUTPUTS}, got {want}")
    sr = _checked("sr", sr)
    if gt is not None:
        gt = _checked("gt", gt)
        if gt.shape != sr.shape or gt.device != sr.device:
            raise HipPathError(f"st_maps: sr and gt must have one shape and one device, got {tuple(sr.shape)} on {sr.device} and "
                               f"{tuple(gt.shape)} on {gt.device}")
    else:
        missing = [w for w in want if w in _NEED_GT]
        if missing:
            raise HipPathError(f"st_maps: {missing} need gt")
    B, _, H, W = sr.shape
    general, _ = st_route(sigma, rho, "st_maps")
    with torch.no_grad(), torch.cuda.device(sr.device):
        def new(*shape):
            return torch.empty(*shape, dtype=torch.float32, device=sr.device)
        bufs = {k: new(B, 3, H, W) for k in ("Sx", "Sgt", "Fx", "Fgt") if k in want}
        if "d" in want:
            bufs["d"] = new(B, H, W)
        if "tile_sums" in want or "distance" in want:
            bufs["tile_sums"] = new(B, workspace_floats(B, H, W) // B)
        p = {k: _abi.ptr(bufs.get(k)) for k in ("Sx", "Sgt", "Fx", "Fgt", "d", "tile_sums")}
        if general:
            _abi.check(_abi.lib().sst_st_general_maps(_abi.ptr(sr), _abi.ptr(gt), p["Sx"], p["Sgt"], p["Fx"], p["Fgt"], p["d"],
                                                      p["tile_sums"], _abi.ptr(new(general_scratch_floats(B, H, W))), B, H, W, float(sigma),
                                                      float(rho), int(bool(normalize)), _abi.stream_ptr()), "sst_st_general_maps")
        else:
            _abi.check(_abi.lib().sst_st_maps(_abi.ptr(sr), _abi.ptr(gt), p["Sx"], p["Sgt"], p["Fx"], p["Fgt"], p["d"], p["tile_sums"],
                                              B, H, W, float(sigma), float(rho), int(bool(normalize)), _abi.stream_ptr()), "sst_st_maps")
        if "distance" in want:
            bufs["distance"] = bufs["tile_sums"].sum(dim=1, dtype=torch.float64) / float(H * W)
    return {k: bufs[k] for k in want}


def structure_tensor(img: Tensor, sigma: float = 0.5, rho: float = 2.0) -> Tensor:
    """[B,3,H,W] RGB -> [B,3,H,W] = (Jxx, Jyy, Jxy) of its gray image (utils.structure_tensor after Grayscale, as the loss
    computes it).  "x" is the height axis: Jxx is the energy of row-to-row variation.  Analysis op, no gradient."""
    return st_maps(img, None, sigma, rho, want=("Sx",))["Sx"]


def st_features(img: Tensor, sigma: float = 0.5, rho: float = 2.0):
    """-> (t, c2, s2), each [B,H,W]: trace t = Jxx + Jyy and the double-angle form c2 = (Jxx - Jyy) / (t + 1e-12),
    s2 = 2 Jxy / (t + 1e-12), well conditioned wherever there is any gradient energy.  c2 = +1: variation along H only, c2 = -1:
    along W only; s2 = +1 for sin(0.5 (col + row)), -1 for sin(0.5 (col - row)).  Analysis op, no gradient."""
    return st_maps(img, None, sigma, rho, want=("Fx",))["Fx"].unbind(dim=1)


def orientation(c2: Tensor, s2: Tensor) -> Tensor:
    """Angle of the dominant gradient direction in (-pi/2, pi/2], measured from the height axis (the reference's "x") towards the
    width axis: 0 for variation along H, +-pi/2 for variation along W."""
    return 0.5 * torch.atan2(s2, c2)


def coherence(c2: Tensor, s2: Tensor) -> Tensor:
    """Anisotropy in [0, 1]: (l_max - l_min) / (l_max + l_min) of the structure tensor; 1 = one orientation only, 0 = isotropic."""
    return torch.hypot(c2, s2)


def st_distance_map(sr: Tensor, gt: Tensor, sigma: float = 0.5, rho: float = 2.0, normalize: bool = True) -> Tensor:
    """-> [B,H,W]: the per-pixel Riemannian distance between the structure tensors of sr and gt (utils.compute_distance), the
    quantity StructureTensorLoss averages.  Analysis op, no gradient."""
    return st_maps(sr, gt, sigma, rho, normalize, want=("d",))["d"]


def st_distance(sr: Tensor, gt: Tensor, sigma: float = 0.5, rho: float = 2.0, normalize: bool = True) -> Tensor:
    """-> [B] fp64 on the device: the per-image mean of st_distance_map; its batch mean is StructureTensorLoss(sr, gt) up to
    summation order.  No host sync.  Analysis op, no gradient."""
    return st_maps(sr, gt, sigma, rho, normalize, want=("distance",))["distance"]
