#!/usr/bin/env python3
"""Golden fixture for the structure-tensor MAPS, FROM THE REFERENCE: utils.structure_tensor of the gray image of x and of gt, and the
per-pixel distance utils.compute_distance(compute_eigenvalues(compute_invS1xS2(S_x, S_gt, normalize))) - the fields
StructureTensorLoss.st_loss (loss.py:399-409) averages - at both (sigma, rho) pairs the HIP kernels build.  Two cases of
2 x 3 x 24 x 20 images: "unit" on the [0, 1] scale with normalize=True, "raw" on the 0..255 scale with normalize=False (so that
eigenvalues of adj(S1) S2 exceed 1).  Stored per case: the inputs as uint8 and, per (sigma, rho), S_x, S_gt [2,3,24,20] and d [2,24,20]
in fp32 - arrays only.  Build container only (needs the reference source, see make_golden.py).
Re-run:  python tests/golden/make_golden_st_maps.py"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import import_reference, save  # noqa: E402

PARAMS = {"s05r20": (0.5, 2.0), "s10r25": (1.0, 2.5)}
CASES = {"unit": (1 / 255, True), "raw": (1.0, False)}        # name -> (scale of the uint8 inputs, normalize)
B, H, W = 2, 24, 20


def main():
    _, _, _, rutils, rloss = import_reference()
    gray = rloss.transforms.Grayscale()
    gen = torch.Generator().manual_seed(777)
    arrs = {}
    for name, (scale, norm) in CASES.items():
        base = torch.rand(B, 3, 6, 5, generator=gen)
        gt = torch.nn.functional.interpolate(base, size=(H, W), mode="bicubic", align_corners=False)
        gt8 = torch.round((gt + 0.05 * torch.randn(gt.shape, generator=gen)).clamp(0, 1) * 255).to(torch.uint8)
        x8 = (gt8.float() + 20 * torch.randn(gt8.shape, generator=gen)).round().clamp(0, 255).to(torch.uint8)
        x, gt = x8.float() * scale, gt8.float() * scale
        p = f"maps/{name}/"
        arrs[p + "x_u8"], arrs[p + "gt_u8"] = x8.numpy(), gt8.numpy()
        arrs[p + "params"] = np.array([scale, float(norm)])
        for tag, (sigma, rho) in PARAMS.items():
            Sx, Sgt, d = [], [], []
            for b in range(B):                                            # the reference works on one (1,H,W) image at a time
                s1 = rutils.structure_tensor(gray(x[b]), sigma=sigma, rho=rho)
                s2 = rutils.structure_tensor(gray(gt[b]), sigma=sigma, rho=rho)
                Sx.append(s1)
                Sgt.append(s2)
                d.append(rutils.compute_distance(rutils.compute_eigenvalues(rutils.compute_invS1xS2(s1, s2, norm))))
            Sx, Sgt, d = torch.stack(Sx), torch.stack(Sgt), torch.stack(d)
            assert Sx.shape == (B, 3, H, W) and d.shape == (B, H, W) and Sx.dtype == torch.float32
            arrs[p + tag + "/Sx"], arrs[p + tag + "/Sgt"], arrs[p + tag + "/d"] = Sx.numpy(), Sgt.numpy(), d.numpy()
            print(f"  maps {name} {tag}: |Sx|={Sx.norm():.4e} |Sgt|={Sgt.norm():.4e} d in [{d.min():.3e}, {d.max():.3e}] mean {d.mean():.6e}")
    save("st_maps", **arrs)


if __name__ == "__main__":
    main()
