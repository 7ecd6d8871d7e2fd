#!/usr/bin/env python3
"""Golden fixture for the structure-tensor loss at the radii only the general path runs (csrc/st_general.hip), FROM THE REFERENCE:
StructureTensorLoss(sigma, rho, normalize) (loss.py:384) at the smallest radii (1, 1), at the widest integration radius next to the
narrowest derivative radius (1, 20), at (4, 8), at (6, 12) with normalize=False (inputs on the 0..255 scale so that eigenvalues of
adj(S1) S2 exceed 1), at the bound (8, 20), there also with x == gt, and at (4, 8) with one NaN in x.  Same recipe and key layout as
make_golden_st_params.py: per case the inputs as uint8 (x = u8 / 255, or u8 itself on the 0..255 scale; x == gt keeps one array), the
reference's fp32 loss, the norm-wise distance of its fp32 d(loss)/d(x) from its fp64 one and where the fp32 one is finite, and its
fp64 loss and d(loss)/d(x) (default dtype fp64, so the reference builds fp64 taps too; the gradient stored in fp32).  Build container
only (needs the reference source, see make_golden.py).  Re-run:  python tests/golden/make_golden_st_general.py"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import import_reference, lowfreq, save  # noqa: E402

NAN_AT = (1, 1, 9, 20)
# name -> (sigma, rho, normalize, kind); images 2 x 3 x 32 x 32
ST_CASES = {
    "s03r03": (0.3, 0.3, True, "noisy"),           # radii (1, 1)
    "s035r50": (0.35, 5.0, True, "noisy"),         # radii (1, 20)
    "s10r20": (1.0, 2.0, True, "noisy"),           # radii (4, 8)
    "s15r30_raw": (1.5, 3.0, False, "scaled"),     # radii (6, 12), normalize=False, 0..255 scale
    "s20r50": (2.0, 5.0, True, "noisy"),           # radii (8, 20): the bound
    "s20r50_eq": (2.0, 5.0, True, "equal"),        # x == gt: disc is exactly 0 in unfused fp32
    "s10r20_nan": (1.0, 2.0, True, "nan"),         # one NaN in x (batch entry 1)
}


def main():
    _, _, _, _, rloss = import_reference()
    gen = torch.Generator().manual_seed(5151)
    arrs = {}
    for name, (sigma, rho, norm, kind) in ST_CASES.items():
        gt8 = torch.round(lowfreq(gen, 2, 32) * 255).to(torch.uint8)
        x8 = (gt8.float() + 20 * torch.randn(gt8.shape, generator=gen)).round().clamp(0, 255).to(torch.uint8)
        if kind == "equal":
            x8 = gt8
        scale = 1.0 if kind == "scaled" else 1 / 255
        x, gt = x8.float() * scale, gt8.float() * scale
        if kind == "nan":
            x[NAN_AT] = float("nan")
        crit = rloss.StructureTensorLoss(sigma=sigma, rho=rho, normalize=norm)
        x = x.clone().requires_grad_(True)
        loss = crit(x, gt)
        (gx,) = torch.autograd.grad(loss, x)
        torch.set_default_dtype(torch.float64)
        x64 = x.detach().double().requires_grad_(True)
        loss64 = crit(x64, gt.double())
        (gx64,) = torch.autograd.grad(loss64, x64)
        torch.set_default_dtype(torch.float32)
        p = f"st/{name}/"
        arrs[p + "gt_u8"] = gt8.numpy()
        if kind != "equal":
            arrs[p + "x_u8"] = x8.numpy()
        arrs[p + "params"] = np.array([sigma, rho, float(norm), scale])
        if kind == "nan":
            arrs[p + "nan_at"] = np.array(NAN_AT)
        arrs[p + "loss"], arrs[p + "loss64"] = loss.detach().numpy(), loss64.detach().numpy()
        fin = torch.isfinite(gx) & torch.isfinite(gx64)
        g32, g64 = gx[fin].double(), gx64[fin]
        arrs[p + "grad_ref_err"] = np.array(float((g32 - g64).norm() / g64.norm()))
        arrs[p + "grad_finite"] = np.packbits(torch.isfinite(gx).numpy())
        arrs[p + "grad64"] = gx64.numpy().astype(np.float32)
        print(f"  st {name}: loss={loss.item():.6e} loss64={loss64.item():.6e} |g|={gx.norm():.4e} |g64|={gx64.norm():.4e}")
    save("st_general", **arrs)


if __name__ == "__main__":
    main()
