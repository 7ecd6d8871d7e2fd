"""Generator criterions on the HIP path.  Mirrors reference loss.py (criterion(sr, gt) -> 0-dim).

MSELoss / L1Loss     nn.MSELoss() of reference config.py:88-90 and its L1 variant, kernels csrc/misc.hip (pixel_loss_*)
StructureTensorLoss  <- reference loss.py:380-413 (+ utils.py:194-280), kernels csrc/st_loss.hip (radii (2,8), (4,10)) and
                        csrc/st_general.hip (every other (sigma, rho) up to radii 8 / 20)
SSIMLoss             1 - mean SSIM, the criterion for the second number validate reports; kernels csrc/ssim_loss.hip
FocalFrequencyLoss   the focal frequency loss (Jiang et al., ICCV 2021): a 2-D DFT and its adjoint; kernels csrc/freq_loss.hip
BackProjectionLoss   the back-projection (LR-consistency) loss of Best-Buddy GANs (Li et al., AAAI 2022): |down(sr) - lr|, the fused
                        antialiased bicubic downscale-and-compare and its adjoint; kernels csrc/bp_loss.hip
GradientLoss         the gradient-magnitude loss of structure-preserving SR (Ma et al., CVPR 2020): |M(sr) - M(gt)| per RGB plane,
                        central-difference or Sobel; kernels csrc/grad_loss.hip
GradientVarianceLoss the gradient-variance loss (Abrahamyan et al., 2022): the MSE between the per-patch variances of the
                        gray Sobel responses; kernels csrc/grad_loss.hip
ArtifactLoss         the artifact-map (locally discriminative) loss of Liang et al. (CVPR 2022): |sr - gt| under a per-pixel weight map
                        from the local variance of the residual, switched off where sr beats the averaged generator's output (a
                        third operand, handed in by the engines); kernels csrc/artifact_loss.hip
ContentLossVGG      <- reference loss.py:11-70, in vgg_loss.py (re-exported here)
BestBuddyLoss / GramLoss / PatchwiseStructureTensorLoss <- reference loss.py:78-228, 292-375, kernels csrc/bb_loss.hip
ContentLossDiscriminator <- reference loss.py:231-289, in disc_loss.py (re-exported here)

The nine pixel-space criteria speak one term protocol (_Term): stand-alone they run under one autograd node
(_TermFn), summed under another (_CriterionSumFn, with the fused pixel + structure-tensor pair _StPixelPair as one more term), and
each of their library entries is launched from one place.
"""
from __future__ import annotations

import ctypes
import os

import torch
from torch import nn

from . import _abi, ops


def _check_pair(who, x, gt, image=True, gt_too=True, on_device=False, second="gt"):
    """The input check of the criteria: an fp32 pair of equal shape; image: [B,3,H,W]; gt_too: gt's dtype counts as well as sr's;
    on_device: both are tensors on one ROCm device, and what is wrong with either is named.  second="lr": the second operand is
    sr's LR image, whose shape is the caller's to check."""
    if on_device:
        for name, t in (("sr", x), (second, gt)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise _abi.HipPathError(f"{who}: {name} must be a tensor on a ROCm device (no CPU fallback)")
            if t.dtype != torch.float32:
                raise _abi.HipPathError(f"{who}: {name} must be fp32, got {t.dtype}")
    bad = x.dtype != torch.float32 or (gt_too and gt.dtype != torch.float32) or (second == "gt" and x.shape != gt.shape)
    if bad or (image and (x.dim() != 4 or x.shape[1] != 3)) or (on_device and x.device != gt.device):
        what = "tensors of equal shape" if not image else "[B,3,H,W] pairs" if second == "gt" else "[B,3,H,W] sr and its LR image"
        raise _abi.HipPathError(f"{who}: expected fp32 {what}"
                                f"{' on one device' if on_device else ''}, got {tuple(x.shape)} / {tuple(gt.shape)}")


def _workspace(entry, *dims, n):
    """sst_<entry>_workspace(dims..., n sizes by reference), checked -> the n sizes (floats) as ints.  Host only."""
    name, sizes = f"sst_{entry}_workspace", [ctypes.c_int64() for _ in range(n)]
    _abi.check(getattr(_abi.lib(), name)(*dims, *map(ctypes.byref, sizes)), name)
    return [v.value for v in sizes]


class _Term(nn.Module):
    """A pixel-space criterion of (sr, gt) as the autograd nodes below drive it - the term protocol:

    _route()                      host only, before anything is launched: which kernels will run (None where there is one route)
    _check(sr, gt)                refuses a pair the kernels do not take (HipPathError); launches and allocates nothing
    _fwd(sr, gt, want_grad, route) -> (raw 0-dim loss, saved): sr, gt contiguous; `saved` is whatever _bwd needs besides sr and gt
                                  and belongs to the call; the reduction workspace lives in self._ws and belongs to the criterion
    _bwd(sr, gt, saved, dsr, g, scale_host, accumulate)   dsr (+)= scale_host * g[0] * d raw / d sr; dsr is the caller's buffer,
                                  g a device scalar"""
    _constant = "gt"          # what the second operand is called where a gradient is asked for it
    wants_reference = False   # True: the engines hand the averaged generator's output in as a third operand (ArtifactLoss)

    def __init__(self):
        super().__init__()
        self._ws = {}

    def _route(self):
        return None

    def _kept(self, saved):
        """`saved` of a forward that ran for a gradient; None (want_grad was False) means the gradient is wanted for the second operand."""
        if saved is None:
            raise _abi.HipPathError(f"{type(self).__name__}: the gradient is taken with respect to sr only ({self._constant} is a constant)")
        return saved

    def forward(self, x, gt):
        want_grad = torch.is_grad_enabled() and isinstance(x, torch.Tensor) and x.requires_grad
        return _TermFn.apply(x, gt, self, want_grad)


class _TermFn(torch.autograd.Function):
    """One _Term stand-alone."""

    @staticmethod
    def forward(ctx, x, gt, term, want_grad):
        route = term._route()
        term._check(x, gt)
        x, gt = x.contiguous(), gt.contiguous()
        loss, ctx.kept = term._fwd(x, gt, want_grad, route)
        ctx.term = term
        ctx.save_for_backward(x, gt)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        x, gt = ctx.saved_tensors
        dx = torch.empty_like(x)
        ctx.term._bwd(x, gt, ctx.kept, dx, grad_out.contiguous().to(torch.float32), 1.0, False)
        return dx, None, None, None


# Dev switch (tests and timing only): send the two built radius pairs down the general path of csrc/st_general.hip as well.
ST_FORCE_GENERAL = os.environ.get("SST_ST_GENERAL", "0") not in ("", "0")


def st_route(sigma, rho, what="StructureTensorLoss"):
    """Which kernels run this (sigma, rho): -> (general, (R1, R2)).  general is False for the two 32 x 32-tile builds (csrc/st_loss.hip,
    csrc/st_maps.hip) and True for the separable path (csrc/st_general.hip, radii up to 8 / 20); beyond that bound HipPathError with
    the library's "... radii (R1,R2) not built".  Host only."""
    r1, r2 = ctypes.c_int(), ctypes.c_int()
    rc = _abi.lib().sst_st_route(float(sigma), float(rho), ctypes.byref(r1), ctypes.byref(r2))
    if rc < 0:
        _abi.check(rc, what)
    return bool(rc) or ST_FORCE_GENERAL, (r1.value, r2.value)


class StructureTensorLoss(_Term):
    """Same constructor and call protocol as reference loss.py:380-413.  Any (sigma, rho) whose radii max(int(4 s + 0.5), 1) are at
    most 8 (sigma) and 20 (rho), i.e. sigma up to about 2.1 and rho up to about 5.1: the pairs with radii (2, 8) and (4, 10) run the
    32 x 32-tile kernels (csrc/st_loss.hip), every other pair the separable path (csrc/st_general.hip); beyond the bound HipPathError."""

    def __init__(self, sigma: float = 0.5, rho: float = 2.0, normalize: bool = True):
        super().__init__()
        self.sigma = sigma
        self.rho = rho
        self.normalize = normalize

    def _route(self):
        return st_route(self.sigma, self.rho)

    def _check(self, x, gt):
        _check_pair("StructureTensorLoss", x, gt)

    def _tile_ws(self, x):
        """The tile kernels' partials / last-arriver counter, keyed by device and shape -> (floats of the partials, partials, counter)."""
        B, _, H, W = x.shape
        n, = _workspace("st_loss", B, H, W, n=1)
        return (n, *ops.reduction_ws(self._ws, (x.device, B, H, W), n))

    def _fwd(self, x, gt, want_grad, route):
        """gS = d(per-pixel distance) / d(structure tensor of sr) is written either way: it belongs to the call, and with what
        else is saved it says which route ran.  Algorithmic bytes: forward reads sr + gt, backward writes d(sr) -
        3 x 3*H*W*4 B per image in all (the planes in between are the general path's own traffic)."""
        general, radii = route
        B, _, H, W = x.shape
        cfg, ws = (float(self.sigma), float(self.rho)), self._ws
        gS = torch.empty_like(x)
        loss = torch.empty((), device=x.device, dtype=torch.float32)
        if not general:
            _, partials, counter = self._tile_ws(x)
            args = (_abi.ptr(x), _abi.ptr(gt), _abi.ptr(loss), _abi.ptr(gS), _abi.ptr(partials), _abi.ptr(counter), B, H, W, *cfg,
                    int(bool(self.normalize)))
            ops._launch_hbm(_abi.lib().sst_st_loss_fwd, args, "sst_st_loss_fwd", "st_loss_fwd_kernel", 2.0 * x.numel() * 4, (x, gt, loss, gS, ws))
            return loss, (cfg, gS)
        # general route: scratch planes next to partials and counter, keyed by the radii as well (a warm-up call allocates them before
        # a graph capture); they only live inside one entry point.  The saved planes (Ix, Iy of sr) belong to the call, like gS.
        n_scratch, n_saved, n_part = _workspace("st_general", B, H, W, n=3)
        partials, counter, scratch = ops.reduction_ws(ws, (x.device, B, H, W, radii), n_part, "general_", scratch=n_scratch)
        planes = torch.empty(n_saved, device=x.device, dtype=torch.float32)
        args = (_abi.ptr(x), _abi.ptr(gt), _abi.ptr(loss), _abi.ptr(gS), _abi.ptr(planes), _abi.ptr(scratch), _abi.ptr(partials),
                _abi.ptr(counter), B, H, W, *cfg, int(bool(self.normalize)))
        ops._launch_hbm(_abi.lib().sst_st_general_fwd, args, "sst_st_general_fwd", "stg_loss_fwd_kernel", 2.0 * x.numel() * 4,
                        (x, gt, loss, gS, planes, ws))
        return loss, (cfg, gS, planes, scratch)

    def _bwd(self, x, gt, saved, dsr, g, scale_host, accumulate):
        cfg, gS, *general = saved                       # what the forward kept says which route it took
        B, _, H, W = x.shape
        if not general:
            args = (_abi.ptr(x), _abi.ptr(gS), _abi.ptr(dsr), _abi.ptr(g), float(scale_host), int(accumulate), B, H, W, *cfg)
            ops._launch_hbm(_abi.lib().sst_st_loss_bwd, args, "sst_st_loss_bwd", "st_loss_bwd_kernel", 1.0 * x.numel() * 4, (x, gS, dsr, g))
            return
        planes, scratch = general
        args = (_abi.ptr(planes), _abi.ptr(gS), _abi.ptr(dsr), _abi.ptr(scratch), _abi.ptr(g), float(scale_host), int(accumulate), B, H, W, *cfg)
        ops._launch_hbm(_abi.lib().sst_st_general_bwd, args, "sst_st_general_bwd", "stg_hadj_out_kernel", 1.0 * x.numel() * 4,
                        (planes, gS, dsr, scratch, g))

    def __repr__(self):
        return f"StructureTensorLoss(sigma={self.sigma}, rho={self.rho}, normalize={self.normalize})"


# ------------------------------------------------------------------------------------------------
SSIM_MIN_SIDE = 11        # the 11-tap window's valid region is empty below it


class SSIMLoss(_Term):
    """1 - mean SSIM(sr, gt): the 11-tap sigma 1.5 Gaussian window over its valid region, C1 = k1^2, C2 = k2^2 for images on the
    0..1 scale - the SSIM validate reports (csrc/metrics.hip) as a criterion, without the uint8 quantisation and the clamp.
    channel "y": one luma plane (65.481 R + 128.553 G + 24.966 B + 16) / 255; "rgb": the mean over the three planes.  fp32
    [B,3,H,W] pairs with H, W >= 11; the gradient is taken with respect to sr only.  Kernels: csrc/ssim_loss.hip."""

    def __init__(self, channel: str = "y", k1: float = 0.01, k2: float = 0.03):
        super().__init__()
        if channel not in ("y", "rgb"):
            raise ValueError(f"SSIMLoss: channel must be 'y' or 'rgb', got {channel!r}")
        for name, k in (("k1", k1), ("k2", k2)):
            if not (isinstance(k, (int, float)) and 0.0 < float(k) < float("inf")):
                raise ValueError(f"SSIMLoss: {name} must be a positive number, got {k!r}")
        self.channel, self.k1, self.k2 = channel, float(k1), float(k2)

    def _check(self, x, gt):
        _check_pair("SSIMLoss", x, gt, on_device=True)
        B, _, H, W = x.shape
        if B < 1 or H < SSIM_MIN_SIDE or W < SSIM_MIN_SIDE:
            raise _abi.HipPathError(f"SSIMLoss: images of {W}x{H} are below the {SSIM_MIN_SIDE}-px minimum of the SSIM window")

    def _fwd(self, x, gt, want_grad, route):
        """want_grad False (no_grad, or sr does not require grad): the gradient maps are neither allocated nor written."""
        B, _, H, W = x.shape
        planes = 1 if self.channel == "y" else 3
        n_maps, n_part = _workspace("ssim_loss", B, H, W, planes, n=2)
        partials, counter = ops.reduction_ws(self._ws, (x.device, B, H, W, planes), n_part)
        maps = torch.empty(n_maps, device=x.device, dtype=torch.float32) if want_grad else None
        loss = torch.empty((), device=x.device, dtype=torch.float32)
        args = (_abi.ptr(x), _abi.ptr(gt), _abi.ptr(loss), _abi.ptr(maps), _abi.ptr(partials), _abi.ptr(counter), B, H, W, planes, self.k1, self.k2)
        # algorithmic bytes: the forward reads sr + gt, the backward writes d(sr)
        ops._launch_hbm(_abi.lib().sst_ssim_loss_fwd, args, "sst_ssim_loss_fwd", "ssim_loss_fwd_kernel", 2.0 * x.numel() * 4,
                        (x, gt, loss, maps, self._ws))
        return loss, (planes, maps) if want_grad else None

    def _bwd(self, x, gt, saved, dsr, g, scale_host, accumulate):
        planes, maps = self._kept(saved)
        B, _, H, W = x.shape
        args = (_abi.ptr(x), _abi.ptr(gt), _abi.ptr(maps), _abi.ptr(dsr), _abi.ptr(g), float(scale_host), int(accumulate), B, H, W, planes)
        ops._launch_hbm(_abi.lib().sst_ssim_loss_bwd, args, "sst_ssim_loss_bwd", "ssim_loss_bwd_kernel", 1.0 * x.numel() * 4,
                        (x, gt, maps, dsr, g))

    def __repr__(self):
        return f"SSIMLoss(channel={self.channel!r}, k1={self.k1}, k2={self.k2})"


# ------------------------------------------------------------------------------------------------
FREQ_MAX_SIDE = 512       # the direct DFT's tables are built for H, W up to this


class FocalFrequencyLoss(_Term):
    """The focal frequency loss (Jiang et al., ICCV 2021) with the published defaults - one patch per image, no averaged spectrum, no
    log weights, per-plane normalisation: with D the orthonormal 2-D DFT of sr - gt per image and RGB plane and e = |D|^2,
    loss = mean(w e), w = sqrt(e)^alpha / max over the plane of sqrt(e)^alpha (NaN -> 0, clamped to [0, 1], a constant for the
    gradient); alpha = 0 is the pixel MSE (Parseval).  fp32 [B,3,H,W] pairs with 1 <= H, W <= 512 of any size (a direct DFT, no radix
    restriction); the gradient is taken with respect to sr only.  Kernels: csrc/freq_loss.hip."""

    def __init__(self, alpha: float = 1.0):
        super().__init__()
        if isinstance(alpha, bool) or not (isinstance(alpha, (int, float)) and 0.0 <= float(alpha) < float("inf")):
            raise ValueError(f"FocalFrequencyLoss: alpha must be a finite number >= 0, got {alpha!r}")
        self.alpha = float(alpha)

    def _check(self, x, gt):
        _check_pair("FocalFrequencyLoss", x, gt, on_device=True)
        B, _, H, W = x.shape
        if B < 1 or not (1 <= H <= FREQ_MAX_SIDE and 1 <= W <= FREQ_MAX_SIDE):
            raise _abi.HipPathError(f"FocalFrequencyLoss: size {H}x{W} not built (1 <= H, W <= {FREQ_MAX_SIDE}, B >= 1)")

    def _fwd(self, x, gt, want_grad, route):
        """want_grad False (no_grad, or sr does not require grad): the weighted spectrum is neither allocated nor written.  The
        transforms' planes (scratch) and the reduction workspace belong to the criterion, keyed by device and shape."""
        B, _, H, W = x.shape
        n_saved, n_scratch, n_part = _workspace("freq_loss", B, H, W, n=3)
        partials, counter, scratch = ops.reduction_ws(self._ws, (x.device, B, H, W), n_part, scratch=n_scratch)
        saved = torch.empty(n_saved, device=x.device, dtype=torch.float32) if want_grad else None
        loss = torch.empty((), device=x.device, dtype=torch.float32)
        args = (_abi.ptr(x), _abi.ptr(gt), _abi.ptr(loss), _abi.ptr(saved), _abi.ptr(scratch), _abi.ptr(partials), _abi.ptr(counter),
                B, H, W, self.alpha)
        # algorithmic bytes: the forward reads sr + gt, the backward writes d(sr)
        ops._launch_hbm(_abi.lib().sst_freq_loss_fwd, args, "sst_freq_loss_fwd", "freq_weight_kernel", 2.0 * x.numel() * 4,
                        (x, gt, loss, saved, self._ws))
        return loss, (saved, scratch) if want_grad else None

    def _bwd(self, x, gt, saved, dsr, g, scale_host, accumulate):
        saved, scratch = self._kept(saved)              # the scratch of the forward's shape, whatever the criterion has seen since
        B, _, H, W = x.shape
        args = (_abi.ptr(saved), _abi.ptr(dsr), _abi.ptr(scratch), _abi.ptr(g), float(scale_host), int(accumulate), B, H, W)
        ops._launch_hbm(_abi.lib().sst_freq_loss_bwd, args, "sst_freq_loss_bwd", "freq_pass_kernel", 1.0 * x.numel() * 4,
                        (saved, dsr, scratch, g))

    def __repr__(self):
        return f"FocalFrequencyLoss(alpha={self.alpha})"


# ------------------------------------------------------------------------------------------------
BP_SCALES = (2, 4, 8)     # the downscaling factors csrc/bp_loss.hip is built for


def bp_transposed_tables(weights, indices, in_size: int):
    """The adjoint of one axis of the clamped-index resampling as gather lists.  weights / indices [out, taps]: a tap table of
    bicubic._contribute (fp32, 0-based).  -> (tw [in_size, N] fp32, ti [in_size, N] int32): row i lists, by ascending output index,
    the (output index, weight) pairs of the outputs that read input i, packed to the front; the rest of a row is (-1, 0).  The
    taps of one output that were clamped onto the same border pixel are merged into one entry (their fp32 weights summed in fp64
    and rounded once): a border list stays as short as an interior one (4) instead of growing to 6 / 10 / 18 at x2 / x4 / x8, and a
    wave that holds a border column walks no longer than its neighbours.  N is the longest list (at least 1).  Host tensors."""
    w, idx = weights.detach().cpu().to(torch.float64).tolist(), indices.detach().cpu().tolist()
    lists = [{} for _ in range(int(in_size))]
    for o, (wrow, irow) in enumerate(zip(w, idx)):
        for wt, i in zip(wrow, irow):
            lists[int(i)][o] = lists[int(i)].get(o, 0.0) + wt
    n = max(1, max(len(l) for l in lists))
    tw, ti = torch.zeros(int(in_size), n, dtype=torch.float32), torch.full((int(in_size), n), -1, dtype=torch.int32)
    for i, l in enumerate(lists):
        if l:
            ti[i, :len(l)] = torch.tensor(sorted(l), dtype=torch.int32)
            tw[i, :len(l)] = torch.tensor([l[o] for o in sorted(l)], dtype=torch.float64).to(torch.float32)
    return tw, ti


class BackProjectionLoss(_Term):
    """The back-projection (LR-consistency) loss of Best-Buddy GANs (Li et al., AAAI 2022): mean |down(sr) - T| ("l1", the paper's)
    or mean (down(sr) - T)^2 ("mse") over batch, RGB and the LR pixels, down = the MATLAB-style antialiased bicubic downscaling by
    `scale` (2, 4 or 8) that makes the LR input (bicubic.Bicubic's tables and the arithmetic of its device kernel).  Called with
    (sr, gt) like every criterion, T = down(gt), rounded to the 1/255 grid when round_target - bit for bit the LR image the dataset
    and the device gathers hand to the generator.  With target="lr" the second argument is the LR image [B,3,H/scale,W/scale]
    itself.  fp32 [B,3,H,W] with H, W >= scale, not necessarily multiples of it; the gradient is taken with respect to sr only.
    Kernels: csrc/bp_loss.hip."""
    _constant = "the target"

    def __init__(self, scale: int = 4, criterion: str = "l1", round_target: bool = True, target: str = "gt"):
        super().__init__()
        if isinstance(scale, bool) or not isinstance(scale, int) or scale not in BP_SCALES:
            raise ValueError(f"BackProjectionLoss: scale must be one of {BP_SCALES}, got {scale!r}")
        if criterion not in ("l1", "mse"):
            raise ValueError(f"BackProjectionLoss: criterion must be 'l1' or 'mse', got {criterion!r}")
        if target not in ("gt", "lr"):
            raise ValueError(f"BackProjectionLoss: target must be 'gt' or 'lr', got {target!r}")
        self.scale, self.criterion, self.round_target, self.target = scale, criterion, bool(round_target), target
        self._tab = {}            # (device, H, W, scale) -> the forward and the transposed tap tables on the device

    def _lr_shape(self, x):
        B, _, H, W = x.shape
        return (B, 3, H // self.scale, W // self.scale)

    def _check(self, x, gt, who="BackProjectionLoss"):
        _check_pair(who, x, gt, on_device=True, second=self.target)
        B, _, H, W = x.shape
        if B < 1 or H < self.scale or W < self.scale:
            raise _abi.HipPathError(f"{who}: images of {W}x{H} are below the {self.scale}-px minimum of scale {self.scale}")
        if self.target == "lr" and tuple(gt.shape) != self._lr_shape(x):
            raise _abi.HipPathError(f"{who}: the LR image of a {tuple(x.shape)} sr at scale {self.scale} is {self._lr_shape(x)}, got "
                                    f"{tuple(gt.shape)}")

    def _tables(self, device, H, W):
        """-> (wy, iy, wx, ix, tw_y, ti_y, tw_x, ti_x) on `device`, built on the host once per (device, H, W, scale): an eager
        warm-up call creates them before a graph capture."""
        key = (device, H, W, self.scale)
        if key not in self._tab:
            from .bicubic import _contribute
            s = 1.0 / self.scale
            w0, i0 = _contribute(H, int(H * s), s)
            w1, i1 = _contribute(W, int(W * s), s)
            fwd = (w0, i0.to(torch.int32), w1, i1.to(torch.int32))
            self._tab[key] = tuple(t.contiguous().to(device) for t in fwd + bp_transposed_tables(w0, i0, H) + bp_transposed_tables(w1, i1, W))
        return self._tab[key]

    def _launch_fwd(self, x, target, want_grad, per_image=False, clamp_sr=False):
        """The one launch site of sst_bp_loss_fwd -> (loss, per-image fp64 [B] or None, saved or None)."""
        B, _, H, W = x.shape
        n_saved, n_part = _workspace("bp_loss", B, H, W, self.scale, n=2)
        wy, iy, wx, ix = self._tables(x.device, H, W)[:4]
        partials, counter = ops.reduction_ws(self._ws, (x.device, B, H, W, self.scale), n_part)
        saved = torch.empty(n_saved, device=x.device, dtype=torch.float32) if want_grad else None
        loss = torch.empty((), device=x.device, dtype=torch.float32)
        per = torch.empty(B, device=x.device, dtype=torch.float64) if per_image else None
        gt, lr = (target, None) if self.target == "gt" else (None, target)
        args = (_abi.ptr(x), _abi.ptr(gt), _abi.ptr(lr), _abi.ptr(loss), _abi.ptr(per), _abi.ptr(saved), _abi.ptr(partials), _abi.ptr(counter),
                _abi.ptr(wy), _abi.ptr(iy), _abi.ptr(wx), _abi.ptr(ix), B, H, W, self.scale, wy.shape[1], wx.shape[1],
                int(self.criterion == "mse"), int(self.round_target), int(bool(clamp_sr)))
        # algorithmic bytes: the forward reads sr + gt (the LR image in lr mode), the backward writes d(sr)
        ops._launch_hbm(_abi.lib().sst_bp_loss_fwd, args, "sst_bp_loss_fwd", "bp_loss_fwd_kernel", (x.numel() + target.numel()) * 4.0,
                        (x, target, loss, saved, self._ws, per, wy, iy, wx, ix))
        return loss, per, saved

    def _fwd(self, x, gt, want_grad, route):
        """want_grad False (no_grad, or sr does not require grad): the saved map is neither allocated nor written."""
        loss, _, saved = self._launch_fwd(x, gt, want_grad)
        return loss, saved

    def _bwd(self, x, gt, saved, dsr, g, scale_host, accumulate):
        saved = self._kept(saved)
        B, _, H, W = x.shape
        tw_y, ti_y, tw_x, ti_x = self._tables(x.device, H, W)[4:]
        args = (_abi.ptr(saved), _abi.ptr(dsr), _abi.ptr(tw_y), _abi.ptr(ti_y), _abi.ptr(tw_x), _abi.ptr(ti_x), _abi.ptr(g), float(scale_host),
                int(accumulate), B, H, W, self.scale, tw_y.shape[1], tw_x.shape[1])
        ops._launch_hbm(_abi.lib().sst_bp_loss_bwd, args, "sst_bp_loss_bwd", "bp_loss_bwd_kernel", 1.0 * x.numel() * 4,
                        (saved, dsr, g, tw_y, ti_y, tw_x, ti_x))

    def __repr__(self):
        extra = ", target='lr'" if self.target == "lr" else ""
        return f"BackProjectionLoss(scale={self.scale}, criterion={self.criterion!r}, round_target={self.round_target}{extra})"


# ------------------------------------------------------------------------------------------------
GRAD_OPERATORS = ("central", "sobel")     # sst_grad_loss_*: op 0, 1
GRAD_CRITERIA = ("l1", "mse")             # crit 0, 1
_NOTHING_SAVED = ()                        # what a forward that ran for a gradient keeps when its backward needs only sr and gt


class GradientLoss(_Term):
    """The pixel-wise gradient loss of structure-preserving SR (Ma et al., CVPR 2020): mean |M(sr) - M(gt)| ("l1") or its square
    ("mse") over batch, RGB planes and pixels, M(I) = sqrt(Gv(I)^2 + Gh(I)^2 + eps) with Gv, Gh the zero-padded 3x3 correlations of a
    plane with the vertical operator - "central" [[0,-1,0],[0,0,0],[0,1,0]] or "sobel" [[-1,-2,-1],[0,0,0],[1,2,1]] - and with its
    transpose.  The derivative of |.| at a tie is 0.  fp32 [B,3,H,W] pairs of any size on one ROCm device; the gradient is taken with
    respect to sr only.  Kernels: csrc/grad_loss.hip."""

    def __init__(self, operator: str = "central", criterion: str = "l1", eps: float = 1e-6):
        super().__init__()
        if operator not in GRAD_OPERATORS:
            raise ValueError(f"GradientLoss: operator must be one of {GRAD_OPERATORS}, got {operator!r}")
        if criterion not in GRAD_CRITERIA:
            raise ValueError(f"GradientLoss: criterion must be one of {GRAD_CRITERIA}, got {criterion!r}")
        if isinstance(eps, bool) or not (isinstance(eps, (int, float)) and 0.0 < float(eps) < float("inf")):
            raise ValueError(f"GradientLoss: eps must be a finite number > 0, got {eps!r}")
        self.operator, self.criterion, self.eps = operator, criterion, float(eps)

    def _modes(self):
        return GRAD_OPERATORS.index(self.operator), GRAD_CRITERIA.index(self.criterion), self.eps

    def _check(self, x, gt):
        _check_pair("GradientLoss", x, gt, on_device=True)
        B, _, H, W = x.shape
        if B < 1 or H < 1 or W < 1:
            raise _abi.HipPathError(f"GradientLoss: empty input {tuple(x.shape)}")

    def _fwd(self, x, gt, want_grad, route):
        """Nothing is saved: the backward recomputes from sr and gt.  A forward that ran for a gradient says so with a marker."""
        B, _, H, W = x.shape
        n_part, = _workspace("grad_loss", B, H, W, n=1)
        partials, counter = ops.reduction_ws(self._ws, (x.device, B, H, W), n_part)
        loss = torch.empty((), device=x.device, dtype=torch.float32)
        args = (_abi.ptr(x), _abi.ptr(gt), _abi.ptr(loss), _abi.ptr(partials), _abi.ptr(counter), B, H, W, *self._modes())
        # algorithmic bytes: the forward reads sr + gt, the backward writes d(sr)
        ops._launch_hbm(_abi.lib().sst_grad_loss_fwd, args, "sst_grad_loss_fwd", "grad_loss_fwd_kernel", 2.0 * x.numel() * 4,
                        (x, gt, loss, None, self._ws))
        return loss, _NOTHING_SAVED if want_grad else None

    def _bwd(self, x, gt, saved, dsr, g, scale_host, accumulate):
        self._kept(saved)
        B, _, H, W = x.shape
        args = (_abi.ptr(x), _abi.ptr(gt), _abi.ptr(dsr), _abi.ptr(g), float(scale_host), int(accumulate), B, H, W, *self._modes())
        ops._launch_hbm(_abi.lib().sst_grad_loss_bwd, args, "sst_grad_loss_bwd", "grad_loss_bwd_kernel", 1.0 * x.numel() * 4,
                        (x, gt, dsr, g))

    def __repr__(self):
        return f"GradientLoss(operator={self.operator!r}, criterion={self.criterion!r}, eps={self.eps})"


GV_MAX_PATCH = 32         # a workgroup of csrc/grad_loss.hip owns whole patches of a 32 x 32 tile


class GradientVarianceLoss(_Term):
    """The gradient-variance loss (Abrahamyan et al., 2022): the zero-padded Sobel responses Gv, Gh of gray = 0.2989 R + 0.587 G +
    0.114 B are cut into non-overlapping patch_size x patch_size patches from the top-left corner (leftover rows and columns belong to
    no patch, but still receive gradient through the taps of patch pixels next to them); with v the unbiased variance of a patch,
    loss = mean((vv(sr) - vv(gt))^2) + mean((vh(sr) - vh(gt))^2) over batch and patches.  fp32 [B,3,H,W] pairs with H, W >= patch_size
    on one ROCm device; the gradient is taken with respect to sr only.  Kernels: csrc/grad_loss.hip."""

    def __init__(self, patch_size: int = 8):
        super().__init__()
        if isinstance(patch_size, bool) or not isinstance(patch_size, int) or not 2 <= patch_size <= GV_MAX_PATCH:
            raise ValueError(f"GradientVarianceLoss: patch_size must be an int from 2 to {GV_MAX_PATCH}, got {patch_size!r}")
        self.patch_size = patch_size

    def _check(self, x, gt):
        _check_pair("GradientVarianceLoss", x, gt, on_device=True)
        B, _, H, W = x.shape
        if B < 1 or H < self.patch_size or W < self.patch_size:
            raise _abi.HipPathError(f"GradientVarianceLoss: images of {W}x{H} are below the patch size {self.patch_size}")

    def _fwd(self, x, gt, want_grad, route):
        """want_grad False (no_grad, or sr does not require grad): the per-patch values are neither allocated nor written."""
        B, _, H, W = x.shape
        n_saved, n_part = _workspace("gv_loss", B, H, W, self.patch_size, n=2)
        partials, counter = ops.reduction_ws(self._ws, (x.device, B, H, W, self.patch_size), n_part)
        saved = torch.empty(n_saved, device=x.device, dtype=torch.float32) if want_grad else None
        loss = torch.empty((), device=x.device, dtype=torch.float32)
        args = (_abi.ptr(x), _abi.ptr(gt), _abi.ptr(loss), _abi.ptr(saved), _abi.ptr(partials), _abi.ptr(counter), B, H, W, self.patch_size)
        # algorithmic bytes: the forward reads sr + gt, the backward writes d(sr)
        ops._launch_hbm(_abi.lib().sst_gv_loss_fwd, args, "sst_gv_loss_fwd", "gv_loss_fwd_kernel", 2.0 * x.numel() * 4,
                        (x, gt, loss, saved, self._ws))
        return loss, saved

    def _bwd(self, x, gt, saved, dsr, g, scale_host, accumulate):
        saved = self._kept(saved)
        B, _, H, W = x.shape
        args = (_abi.ptr(x), _abi.ptr(saved), _abi.ptr(dsr), _abi.ptr(g), float(scale_host), int(accumulate), B, H, W, self.patch_size)
        ops._launch_hbm(_abi.lib().sst_gv_loss_bwd, args, "sst_gv_loss_bwd", "gv_loss_bwd_kernel", 1.0 * x.numel() * 4,
                        (x, saved, dsr, g))

    def __repr__(self):
        return f"GradientVarianceLoss(patch_size={self.patch_size})"


# ------------------------------------------------------------------------------------------------
ARTIFACT_KSIZES = (3, 5, 7, 9, 11)        # the windows csrc/artifact_loss.hip is built for


class _RefTermFn(torch.autograd.Function):
    """One _Term that takes a reference image as a third operand (None: none), stand-alone."""

    @staticmethod
    def forward(ctx, x, gt, ref, term, want_grad):
        route = term._route()
        term._check(x, gt, ref)
        x, gt, ref = x.contiguous(), gt.contiguous(), None if ref is None else ref.contiguous()
        loss, ctx.kept = term._fwd(x, gt, want_grad, route, ref)
        ctx.term = term
        ctx.save_for_backward(x, gt)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        x, gt = ctx.saved_tensors
        dx = torch.empty_like(x)
        ctx.term._bwd(x, gt, ctx.kept, dx, grad_out.contiguous().to(torch.float32), 1.0, False)
        return dx, None, None, None, None


class ArtifactLoss(_Term):
    """The artifact-map (locally discriminative, "LDL") loss of Liang et al., "Details or Artifacts" (CVPR 2022).  With
    r = sum over R, G, B of |gt - sr| and p = ksize // 2: s_b = (unbiased variance of r over image b) ** (1/5), v = the unbiased variance
    of the ksize x ksize window of r around a pixel (r reflect-padded by p), w = s_b * v; loss = mean over B*3*H*W of w * |sr - gt|.
    refine=True: the call takes a third operand ref - the averaged generator's output for the same LR batch (the engines hand it in:
    SOLVER.G_EMA_DECAY > 0) - and w = 0 wherever r < r_e = sum |gt - ref| strictly, i.e. where sr is already closer to gt than ref is;
    ref equal to sr masks nothing.  refine=False ignores a third operand.  The map is a weighting, as the paper describes it: a
    constant of the gradient, d loss / d sr = w * sign(sr - gt) / (3 B H W) with sign(0) = 0; a variant that differentiates through
    the map is out of scope.  fp32 [B,3,H,W] operands with H, W >= p + 1 on one ROCm device, ksize odd from 3 to 11; the gradient is
    taken with respect to sr only.  Kernels: csrc/artifact_loss.hip."""
    _constant = "gt, like ref,"

    def __init__(self, ksize: int = 7, refine: bool = True):
        super().__init__()
        if isinstance(ksize, bool) or not isinstance(ksize, int) or ksize not in ARTIFACT_KSIZES:
            raise ValueError(f"ArtifactLoss: ksize must be an odd int from {ARTIFACT_KSIZES[0]} to {ARTIFACT_KSIZES[-1]}, got {ksize!r}")
        self.ksize, self.refine = ksize, bool(refine)

    @property
    def wants_reference(self):
        return self.refine

    def forward(self, x, gt, ref=None):
        want_grad = torch.is_grad_enabled() and isinstance(x, torch.Tensor) and x.requires_grad
        return _RefTermFn.apply(x, gt, ref if self.refine else None, self, want_grad)

    def _check(self, x, gt, ref=None):
        _check_pair("ArtifactLoss", x, gt, on_device=True)
        if self.refine:
            if ref is None:
                raise _abi.HipPathError("ArtifactLoss: refine=True takes the averaged generator's output as a third operand (the engines "
                                        "hand it in when SOLVER.G_EMA_DECAY > 0); without one, construct it with refine=False")
            if not isinstance(ref, torch.Tensor) or not ref.is_cuda:
                raise _abi.HipPathError("ArtifactLoss: ref must be a tensor on a ROCm device (no CPU fallback)")
            if ref.dtype != torch.float32 or ref.shape != x.shape or ref.device != x.device:
                raise _abi.HipPathError(f"ArtifactLoss: ref must be fp32, of sr's shape and on sr's device, got {ref.dtype} "
                                        f"{tuple(ref.shape)} for sr {tuple(x.shape)}")
        B, _, H, W = x.shape
        if B < 1 or H < self.ksize // 2 + 1 or W < self.ksize // 2 + 1:
            raise _abi.HipPathError(f"ArtifactLoss: images of {W}x{H} are below the {self.ksize // 2 + 1}-px minimum of the reflected "
                                    f"{self.ksize}x{self.ksize} window")

    def _fwd(self, x, gt, want_grad, route, ref=None):
        """want_grad False (no_grad, or sr does not require grad): the w map is neither allocated nor written.  Two reduction
        workspaces: "stat_" for the per-image variance (its partials end in the B global weights), the plain one for the loss."""
        B, _, H, W = x.shape
        n_map, n_stat, n_part = _workspace("artifact_loss", B, H, W, self.ksize, n=3)
        key = (x.device, B, H, W, self.ksize)
        partials, counter = ops.reduction_ws(self._ws, key, n_part)
        stats, stat_counter = ops.reduction_ws(self._ws, key, n_stat, "stat_")
        wmap = torch.empty(n_map, device=x.device, dtype=torch.float32) if want_grad else None
        loss = torch.empty((), device=x.device, dtype=torch.float32)
        args = (_abi.ptr(x), _abi.ptr(gt), _abi.ptr(ref), _abi.ptr(loss), _abi.ptr(wmap), _abi.ptr(stats), _abi.ptr(stat_counter),
                _abi.ptr(partials), _abi.ptr(counter), B, H, W, self.ksize)
        # algorithmic bytes: the forward reads sr + gt (+ ref), the backward writes d(sr)
        ops._launch_hbm(_abi.lib().sst_artifact_loss_fwd, args, "sst_artifact_loss_fwd", "artifact_loss_fwd_kernel",
                        (2.0 if ref is None else 3.0) * x.numel() * 4, (x, gt, loss, wmap, self._ws, ref))
        return loss, (wmap,) if want_grad else None

    def _bwd(self, x, gt, saved, dsr, g, scale_host, accumulate):
        wmap, = self._kept(saved)
        B, _, H, W = x.shape
        args = (_abi.ptr(x), _abi.ptr(gt), _abi.ptr(wmap), _abi.ptr(dsr), _abi.ptr(g), float(scale_host), int(accumulate), B, H, W, self.ksize)
        ops._launch_hbm(_abi.lib().sst_artifact_loss_bwd, args, "sst_artifact_loss_bwd", "artifact_loss_bwd_kernel", 1.0 * x.numel() * 4,
                        (x, gt, wmap, dsr, g))

    def __repr__(self):
        return f"ArtifactLoss(ksize={self.ksize}, refine={self.refine})"


# ------------------------------------------------------------------------------------------------
class _PixelLoss(_Term):
    mode = None               # sst_pixel_loss_*: 0 MSE, 1 L1

    def _check(self, x, gt):
        _check_pair("pixel loss", x, gt, image=False, gt_too=False)

    def _fwd(self, x, gt, want_grad, route):
        return ops.pixel_loss_fwd(x, gt, self.mode, self._ws), None

    def _bwd(self, x, gt, saved, dsr, g, scale_host, accumulate):
        ops.pixel_loss_bwd(x, gt, self.mode, scale_dev=g, scale_host=scale_host, out=dsr, accumulate=accumulate)


class MSELoss(_PixelLoss):
    """nn.MSELoss() of reference config.py:88-90 on the HIP path."""
    mode = 0


class L1Loss(_PixelLoss):
    """Pixel-L1 variant named by BASELINE.json configs[0] (one-line config change in the reference)."""
    mode = 1


# ------------------------------------------------------------------------------------------------
FUSE_PIXEL_INTO_ST = os.environ.get("SST_FUSE_PIXEL_ST", "1") != "0"


class _StPixelPair:
    """A tile-route StructureTensorLoss and a pixel criterion as one term: the pixel criterion rides along in the structure-tensor
    kernels - same reads of sr / gt, two launches less per step (forward and backward).  Two raw values, two host scales; the
    workspace is the structure-tensor term's."""

    def __init__(self, st, pixel):
        self.st, self.pixel = st, pixel

    def _fwd(self, x, gt, want_grad, route):
        st, ws = self.st, self.st._ws
        B, _, H, W = x.shape
        cfg = (float(st.sigma), float(st.rho))
        n, partials, counter = st._tile_ws(x)
        pix_partials, _ = ops.reduction_ws(ws, (x.device, n), n, "pix_")
        gS = torch.empty_like(x)
        loss = torch.empty((), device=x.device, dtype=torch.float32)
        pix = torch.empty((), device=x.device, dtype=torch.float32)
        args = (_abi.ptr(x), _abi.ptr(gt), _abi.ptr(loss), _abi.ptr(gS), _abi.ptr(partials), _abi.ptr(counter), _abi.ptr(pix),
                _abi.ptr(pix_partials), self.pixel.mode, B, H, W, *cfg, int(bool(st.normalize)))
        ops._launch_hbm(_abi.lib().sst_st_pixel_loss_fwd, args, "sst_st_pixel_loss_fwd", "st_loss_fwd_kernel", 2.0 * x.numel() * 4,
                        (x, gt, loss, gS, ws, pix))
        return (loss, pix), (cfg, gS)

    def _bwd(self, x, gt, saved, dsr, g, scale_host, accumulate):
        cfg, gS = saved
        B, _, H, W = x.shape
        args = (_abi.ptr(x), _abi.ptr(gt), _abi.ptr(gS), _abi.ptr(dsr), _abi.ptr(g), float(scale_host[0]), float(scale_host[1]),
                self.pixel.mode, int(accumulate), B, H, W, *cfg)
        ops._launch_hbm(_abi.lib().sst_st_pixel_loss_bwd, args, "sst_st_pixel_loss_bwd", "st_loss_bwd_kernel", 1.0 * x.numel() * 4,
                        (x, gt, gS, dsr, g))


class _CriterionSumFn(torch.autograd.Function):
    """total = sum_i w_i * criterion_i(sr, gt) for HIP-path criterions, as ONE autograd node: the weighted values and the
    total come out of one tiny kernel, and the backward kernels of the terms accumulate into one d(sr) buffer with the
    weight folded into their scale - no per-term mul / add launches (reference train.py:129-140 / warmup.py:79-86 loop)."""

    @staticmethod
    def forward(ctx, sr, gt, terms, weights):
        _check_pair("criterion sum", sr, gt, image=False, gt_too=False)
        sr, gt = sr.contiguous(), gt.contiguous()
        routes = [t._route() for t in terms]            # every host-side decision and refusal comes before the first launch
        for t in terms:
            t._check(sr, gt)
        steps = [(t, (i,)) for i, t in enumerate(terms)]                   # (what runs, the terms it computes)
        # one structure-tensor term on the tile route + one pixel term (the step's usual pair) run as _StPixelPair (the fused
        # kernels are the tile builds': a structure-tensor term on the general route runs unfused)
        st = [i for i, t in enumerate(terms) if isinstance(t, StructureTensorLoss)]
        px = [i for i, t in enumerate(terms) if isinstance(t, _PixelLoss)]
        if FUSE_PIXEL_INTO_ST and len(st) == 1 and len(px) == 1 and not routes[st[0]][0]:
            pair = (st[0], px[0])
            steps = [(_StPixelPair(terms[st[0]], terms[px[0]]), pair)] + [s for s in steps if s[1][0] not in pair]
        raw, kept = [None] * len(terms), []
        for op, idx in steps:
            out, k = op._fwd(sr, gt, True, routes[idx[0]])
            kept.append(k)
            for i, r in zip(idx, out if len(idx) > 1 else (out,)):
                raw[i] = r
        total, weighted = ops.weighted_sum(raw, weights, True)
        ctx.steps, ctx.kept, ctx.weights = steps, kept, [float(w) for w in weights]
        ctx.save_for_backward(sr, gt)
        ctx.mark_non_differentiable(weighted)
        ctx.set_materialize_grads(False)                 # no zeros kernel for the gradient slot of `weighted`
        return total, weighted

    @staticmethod
    def backward(ctx, grad_total, _grad_weighted):
        sr, gt = ctx.saved_tensors
        g = grad_total.contiguous().to(torch.float32)
        dsr = torch.empty_like(sr)
        for n, ((op, idx), k) in enumerate(zip(ctx.steps, ctx.kept)):
            w = [ctx.weights[i] for i in idx]
            op._bwd(sr, gt, k, dsr, g, w if len(idx) > 1 else w[0], n > 0)
        return dsr, None, None, None


def fusable(criterion) -> bool:
    """Whether engine._criterion_total hands the criterion to criterion_sum.  SSIMLoss speaks the term protocol but stays outside:
    taking it in changes the launches of a step with an SSIM term."""
    return isinstance(criterion, (MSELoss, L1Loss, StructureTensorLoss))


def criterion_sum(sr, gt, terms, weights):
    """-> (total, weighted values [len(terms)]) for fusable() criterions of (sr, gt)."""
    return _CriterionSumFn.apply(sr, gt, list(terms), list(weights))


# ------------------------------------------------------------------------------------------------
def _torch_bicubic_taps(in_size: int, out_size: int, device, scale=None):
    """Tap tables of F.interpolate(mode='bicubic', align_corners=False) (A = -0.75, 4 taps, border indices clamped):
    -> (weights [out, 4] fp32, indices [out, 4] int32).  scale: source pixels per output pixel; F.interpolate(scale_factor=f) maps
    coordinates with 1 / f, not with in_size / out_size (they differ when in_size * f is not an integer)."""
    A = -0.75
    o = torch.arange(out_size, dtype=torch.float64)
    src = (o + 0.5) * (float(scale) if scale is not None else in_size / out_size) - 0.5
    x0 = torch.floor(src)
    t = src - x0

    def cc1(x):
        return ((A + 2) * x - (A + 3)) * x * x + 1

    def cc2(x):
        return ((A * x - 5 * A) * x + 8 * A) * x - 4 * A

    w = torch.stack([cc2(t + 1), cc1(t), cc1(1 - t), cc2(2 - t)], dim=1).to(torch.float32)
    idx = (x0.unsqueeze(1) + torch.arange(-1, 3, dtype=torch.float64).unsqueeze(0)).clamp(0, in_size - 1).to(torch.int32)
    return w.contiguous().to(device), idx.contiguous().to(device)


def _gt_pyramid(gt, cache, nps, extract):
    """The candidate side of the patch losses: extract(image, h, w, offset) on GT at full resolution, then on GT at 1/2 and 1/4
    resolution (F.interpolate(scale_factor=0.5 / 0.25, mode='bicubic'): floor sizes, coordinates mapped with the factor), the offset
    running by nps = patches per level.  The tap tables are cached in `cache` per (device, H, W)."""
    B, _, H, W = gt.shape
    key = (gt.device, H, W)
    if cache.get("key") != key:
        cache["key"] = key
        cache["taps"] = [(_torch_bicubic_taps(H, H // s, gt.device, s), _torch_bicubic_taps(W, W // s, gt.device, s)) for s in (2, 4)]
    extract(gt, H, W, 0)
    off = nps[0]
    for k, s in enumerate((2, 4)):
        (wy, iy), (wx, ix) = cache["taps"][k]
        small = torch.empty(B, 3, H // s, W // s, device=gt.device, dtype=torch.float32)
        _abi.check(_abi.lib().sst_bicubic(_abi.ptr(gt), _abi.ptr(small), _abi.ptr(wy), _abi.ptr(iy), _abi.ptr(wx), _abi.ptr(ix), B * 3, H, W,
                                          H // s, W // s, 4, 4, 0, _abi.stream_ptr()), "sst_bicubic")
        extract(small, H // s, W // s, off)
        off += nps[k + 1]


class _BestBuddyGeneralFn(torch.autograd.Function):
    """BestBuddyLoss with any patch geometry (ksize <= 6, pad, stride; reference loss.py:86,116-134) and either matching distance
    (utils.py:157-191): patch tables in global memory (sst_bbg_unfold), tiled matching (sst_bbg_match), the unfold's adjoint for the
    gradient (sst_bbg_fold) - csrc/bb_loss.hip."""

    @staticmethod
    def forward(ctx, x, gt, alpha, beta, l2, ksize, pad, stride, dist_l1, cache):
        _check_pair("BestBuddyLoss", x, gt, gt_too=False)
        B, _, H, W = x.shape
        x, gt = x.contiguous(), gt.contiguous()
        lib, dev = _abi.lib(), x.device
        nps = [lib.sst_bbg_patches(H // s, W // s, ksize, pad, stride) for s in (1, 2, 4)]
        if min(nps) <= 0:
            raise _abi.HipPathError(f"BestBuddyLoss: a {ksize}x{ksize} patch (pad {pad}) does not fit the 1/4-resolution image")
        D, ncand, np_ = 3 * ksize * ksize, sum(nps), nps[0]
        cand = torch.empty(B, ncand, D, device=dev, dtype=torch.float32)
        cnrm = torch.empty(B, ncand, device=dev, dtype=torch.float32)
        st = _abi.stream_ptr()
        _gt_pyramid(gt, cache, nps, lambda img, h, w, off: _abi.check(
            lib.sst_bbg_unfold(_abi.ptr(img), _abi.ptr(cand), _abi.ptr(cnrm), B, h, w, ksize, pad, stride, ncand, off, st), "sst_bbg_unfold"))
        srf = torch.empty(B, np_, D, device=dev, dtype=torch.float32)
        _abi.check(lib.sst_bbg_unfold(_abi.ptr(x), _abi.ptr(srf), None, B, H, W, ksize, pad, stride, np_, 0, st), "sst_bbg_unfold")
        ind = torch.empty(B, np_, device=dev, dtype=torch.int32)
        gfeat = torch.empty(B, np_, D, device=dev, dtype=torch.float32)
        partials = torch.empty(lib.sst_bbg_blocks(B, np_), device=dev, dtype=torch.float32)
        _abi.check(lib.sst_bbg_match(_abi.ptr(srf), _abi.ptr(cand), _abi.ptr(cnrm), _abi.ptr(ind), _abi.ptr(gfeat), _abi.ptr(partials), B, np_, ncand,
                                     D, float(alpha), float(beta), int(l2), int(dist_l1), st), "sst_bbg_match")
        dsr = torch.empty_like(x)
        _abi.check(lib.sst_bbg_fold(_abi.ptr(gfeat), _abi.ptr(dsr), B, H, W, ksize, pad, stride, st), "sst_bbg_fold")
        ctx.save_for_backward(dsr)
        ctx.mark_non_differentiable(ind)
        return partials.sum(), ind

    @staticmethod
    def backward(ctx, grad_out, _grad_ind):
        (dsr,) = ctx.saved_tensors
        return dsr * grad_out, None, None, None, None, None, None, None, None, None


class _BestBuddyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gt, alpha, beta, l2, cache, gram=0, st_mats=None, dist_l1=0):
        _check_pair("BestBuddyLoss / GramLoss", x, gt, gt_too=False)
        B, _, H, W = x.shape
        if H % 12 or W % 12:
            raise _abi.HipPathError("BestBuddyLoss: H and W must be multiples of 12 (3x3 patches at scales 1, 1/2, 1/4)")
        x, gt = x.contiguous(), gt.contiguous()
        lib, dev = _abi.lib(), x.device
        nps = [(H // s // 3) * (W // s // 3) for s in (1, 2, 4)]
        ncand = sum(nps)
        cand = torch.empty(B, ncand, lib.sst_bb_feature_dim(int(gram)), device=dev, dtype=torch.float32)
        cnrm = torch.empty(B, ncand, device=dev, dtype=torch.float32)
        st = _abi.stream_ptr()
        _gt_pyramid(gt, cache, nps, lambda img, h, w, off: _abi.check(
            lib.sst_bb_patches(_abi.ptr(img), _abi.ptr(cand), _abi.ptr(cnrm), B, h, w, ncand, off, int(gram), _abi.ptr(st_mats), st), "sst_bb_patches"))
        ind = torch.empty(B, nps[0], device=dev, dtype=torch.int32)
        dsr = torch.empty_like(x)
        partials = torch.empty(lib.sst_bb_blocks(B, H, W), device=dev, dtype=torch.float32)
        _abi.check(lib.sst_bb_match_dist(_abi.ptr(x), _abi.ptr(cand), _abi.ptr(cnrm), _abi.ptr(ind), _abi.ptr(dsr), _abi.ptr(partials), B, H, W,
                                         ncand, float(alpha), float(beta), int(l2), int(gram), _abi.ptr(st_mats), int(dist_l1), st), "sst_bb_match")
        ctx.save_for_backward(dsr)
        ctx.mark_non_differentiable(ind)
        return partials.sum(), ind

    @staticmethod
    def backward(ctx, grad_out, _grad_ind):
        (dsr,) = ctx.saved_tensors
        return dsr * grad_out, None, None, None, None, None, None, None, None


def _patch_modes(dist_norm: str, criterion: str, verb: str = "implmented"):
    """The dist_norm / criterion arguments of the three patch losses -> (dist_l1, l2), refused in the reference's words."""
    if dist_norm not in ("l1", "l2"):
        raise NotImplementedError("%s norm has not been supported." % dist_norm)          # utils.py:189
    if criterion not in ("l1", "l2", "mse"):
        raise NotImplementedError("%s criterion has not been %s." % (criterion, verb))
    return int(dist_norm == "l1"), criterion != "l1"


class BestBuddyLoss(nn.Module):
    """Reference loss.py:78-142 (Best-Buddy GAN loss) on the HIP path.  Same constructor: any ksize (<= 6) / pad / stride and
    dist_norm 'l1' or 'l2', criterion 'l1' or 'l2' / 'mse'.  The reference's default geometry (ksize 3, pad 0, stride 3, images with
    H, W multiples of 12) runs the register-resident kernels, everything else the table-based ones (_BestBuddyGeneralFn)."""

    def __init__(self, alpha: float = 1.0, beta: float = 1.0, ksize: int = 3, pad: int = 0, stride: int = 3, dist_norm: str = "l2",
                 criterion: str = "l1") -> None:
        super().__init__()
        if not (1 <= int(ksize) <= 6 and int(pad) >= 0 and int(stride) >= 1):
            raise NotImplementedError("BestBuddyLoss on the HIP path: 1 <= ksize <= 6, pad >= 0, stride >= 1")
        self._dl1, self.l2 = _patch_modes(dist_norm, criterion)
        self.alpha, self.beta, self.ksize, self.pad, self.stride, self.dist_norm = alpha, beta, ksize, pad, stride, dist_norm
        self._cache = {}
        self.last_index = None          # [B, n_patches] int32: the selected candidate per SR patch (diagnostics / tests)

    def forward(self, x, gt):
        default = (self.ksize, self.pad, self.stride) == (3, 0, 3) and x.shape[2] % 12 == 0 and x.shape[3] % 12 == 0
        if default:
            loss, ind = _BestBuddyFn.apply(x, gt, float(self.alpha), float(self.beta), self.l2, self._cache, 0, None, self._dl1)
        else:
            loss, ind = _BestBuddyGeneralFn.apply(x, gt, float(self.alpha), float(self.beta), self.l2, int(self.ksize), int(self.pad),
                                                  int(self.stride), self._dl1, self._cache)
        self.last_index = ind
        return loss


class GramLoss(nn.Module):
    """Reference loss.py:145-228 (best-buddy matching on the 3x3 gram matrix of every 3x3 patch) on the HIP path.  Same
    constructor; supported: ksize 3 (the reference's reshape to 9 features assumes it, loss.py:200), dist_norm 'l1' or 'l2',
    criterion 'l1' or 'l2' / 'mse'."""

    def __init__(self, alpha: float = 1.0, beta: float = 1.0, ksize: int = 3, dist_norm: str = "l2", criterion: str = "l1") -> None:
        super().__init__()
        if ksize != 3:
            raise NotImplementedError("GramLoss on the HIP path: ksize=3 only")
        self._dl1, self.l2 = _patch_modes(dist_norm, criterion)
        self.alpha, self.beta, self.ksize, self.dist_norm = alpha, beta, ksize, dist_norm
        self._cache = {}
        self.last_index = None

    def forward(self, x, gt):
        loss, ind = _BestBuddyFn.apply(x, gt, float(self.alpha), float(self.beta), self.l2, self._cache, 1, None, self._dl1)
        self.last_index = ind
        return loss


def _patch_st_matrices(sigma: float, rho: float, device):
    """The three 9x9 linear maps of utils.py:212-233 on a zero-padded 3x3 image, row-major [out pixel][in pixel]:
    Ix = Ax g (derivative taps along H, Gaussian along W), Iy = Ay g, J = K (product)  -> device tensor [3*81]."""
    def taps(s, also_dg=False):                         # utils.py:194-208 (fp32 taps from an int64 arange)
        radius = max(int(4 * s + 0.5), 1)
        xs = torch.arange(-radius, radius + 1)
        s2 = s * s + 1e-12
        phi = torch.exp(-0.5 / s2 * xs ** 2)
        phi = phi / phi.sum()
        return (phi, phi * -xs / s2, radius) if also_dg else (phi, radius)

    g, dg, r1 = taps(sigma, True)
    k, r2 = taps(rho)

    def mat(kv, kh, r):                                  # out (y,x) <- in (y',x'):  kv[y'-y+r] * kh[x'-x+r]
        m = torch.zeros(9, 9)
        for y in range(3):
            for x in range(3):
                for yy in range(3):
                    for xx in range(3):
                        a, b = yy - y + r, xx - x + r
                        if 0 <= a <= 2 * r and 0 <= b <= 2 * r:
                            m[y * 3 + x, yy * 3 + xx] = kv[a] * kh[b]
        return m

    return torch.cat([mat(dg, g, r1).reshape(-1), mat(g, dg, r1).reshape(-1), mat(k, k, r2).reshape(-1)]).to(torch.float32).to(device)


class PatchwiseStructureTensorLoss(nn.Module):
    """Reference loss.py:292-375 (best-buddy matching on the normalised structure tensor of every 3x3 patch) on the HIP path.
    Same constructor; supported: ksize 3, dist_norm 'l1' or 'l2', criterion 'l1' or 'l2' / 'mse'."""

    def __init__(self, sigma: float = 0.5, rho: float = 2, alpha: float = 1.0, beta: float = 1.0, ksize: int = 3, dist_norm: str = "l2",
                 criterion: str = "l1"):
        super().__init__()
        if ksize != 3:
            raise NotImplementedError("PatchwiseStructureTensorLoss on the HIP path: ksize=3 only")
        self._dl1, self.l2 = _patch_modes(dist_norm, criterion, "supported")
        self.sigma, self.rho, self.alpha, self.beta, self.ksize, self.dist_norm = sigma, rho, alpha, beta, ksize, dist_norm
        self._cache = {}
        self._mats = None
        self.last_index = None

    def forward(self, x, gt):
        if self._mats is None or self._mats.device != x.device:
            self._mats = _patch_st_matrices(float(self.sigma), float(self.rho), x.device)
        loss, ind = _BestBuddyFn.apply(x, gt, float(self.alpha), float(self.beta), self.l2, self._cache, 2, self._mats, self._dl1)
        self.last_index = ind
        return loss


class _BceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target_value):
        logits = logits.contiguous()
        ctx.save_for_backward(logits)
        ctx.t = target_value
        loss, _ = ops.bce_logits(logits, target_value, want_loss=True)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        (logits,) = ctx.saved_tensors
        _, dl = ops.bce_logits(logits, ctx.t, want_loss=False, want_grad=True, scale_dev=grad_out.contiguous())
        return dl, None


class _AdvTermFn(torch.autograd.Function):
    """total + w * BCEWithLogits(logits, t) -> (new total, w * BCE): the generator's adversarial term (reference train.py:136-140:
    `loss = criterion(D(sr), real) * weight; total += loss`) as one autograd node - one tiny launch for scaling + sum in the forward,
    and the weight folded into the scale of the BCE gradient in the backward (no mul / add launches of autograd)."""

    @staticmethod
    def forward(ctx, total, logits, t, w):
        logits = logits.contiguous()
        raw, _ = ops.bce_logits(logits, t, want_loss=True)
        out, weighted = ops.weighted_sum([total.contiguous(), raw], [1.0, w], True)
        ctx.save_for_backward(logits)
        ctx.t, ctx.w = t, float(w)
        ctx.mark_non_differentiable(weighted)
        ctx.set_materialize_grads(False)
        return out, weighted

    @staticmethod
    def backward(ctx, g, _gw):
        (logits,) = ctx.saved_tensors
        _, dl = ops.bce_logits(logits, ctx.t, want_loss=False, want_grad=True, scale_dev=g.contiguous(), scale_host=ctx.w)
        return g, dl, None, None


def adversarial_term(total, logits, crit, label, weight):
    """-> (total + weight * crit(logits, label), weight * crit(...) detached) for crit = BCEWithLogitsLoss (see _AdvTermFn)."""
    out, weighted = _AdvTermFn.apply(total, logits, crit.label_value(label), weight)
    return out, weighted[1]


class BCEWithLogitsLoss(nn.Module):
    """nn.BCEWithLogitsLoss() of reference config.py:71-73 / train.py:59.  The reference always calls it
    with a constant-filled label tensor (train.py:113-114: 0.9 or 0); the label value is read once on the
    host when the label tensor is first seen (cached by identity), so there is no per-step sync."""

    def __init__(self):
        super().__init__()
        self._label_cache = {}

    def forward(self, logits, label):
        return _BceFn.apply(logits, self.label_value(label))

    def label_value(self, label):
        if isinstance(label, (int, float)):
            t = float(label)
        else:
            key = (label.data_ptr(), label._version, tuple(label.shape))
            t = self._label_cache.get(key)
            if t is None:
                t = float(label.flatten()[0].item())
                if not bool((label == t).all().item()):
                    raise _abi.HipPathError("BCEWithLogitsLoss (HIP path): label tensor must be constant-filled "
                                            "(reference train.py:113-114 uses full([B,1], 0.9) / zeros)")
                self._label_cache = {key: t}
        return t


from .vgg_loss import ContentLossVGG  # noqa: E402,F401  (reference loss.py:11)
from .disc_loss import ContentLossDiscriminator  # noqa: E402,F401  (reference loss.py:231)
