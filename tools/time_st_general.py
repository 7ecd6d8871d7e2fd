#!/usr/bin/env python3
"""What the general structure-tensor path (csrc/st_general.hip: separable passes over whole planes, radii up to 8 / 20) costs next to
the 32 x 32-tile kernels (csrc/st_loss.hip), in one process: StructureTensorLoss forward + backward at B = 16, 96 px, replayed back
to back from a hipGraph, us per forward + backward.

    rows   tile     (0.5, 2.0)   radii (2, 8)    the tile build: the yardstick
           general  (0.5, 2.0)   radii (2, 8)    the same pair forced down the general path (loss.ST_FORCE_GENERAL)
           general  (1.0, 2.0)   radii (4, 8)
           general  (1.5, 3.0)   radii (6, 12)
           general  (2.0, 5.0)   radii (8, 20)   the bound

Prints one JSON line.  Under its own time limit:

    timeout -k 10 120 python tools/time_st_general.py
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "srgan-st_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from time_ema import replay_us  # noqa: E402

ROWS = [("tile", 0.5, 2.0), ("general", 0.5, 2.0), ("general", 1.0, 2.0), ("general", 1.5, 3.0), ("general", 2.0, 5.0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=96)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    from srganst import loss as sl
    g = torch.Generator().manual_seed(1)
    gt = torch.rand(a.batch, 3, a.size, a.size, generator=g)
    x = (gt + 0.08 * torch.randn(gt.shape, generator=g)).clamp(0, 1).cuda().requires_grad_(True)
    gt = gt.cuda()
    out = {"device": torch.cuda.get_device_name(0), "batch": a.batch, "size": a.size, "rows": []}
    for path, sigma, rho in ROWS:
        sl.ST_FORCE_GENERAL = path == "general"
        general, radii = sl.st_route(sigma, rho)
        assert general == (path == "general")
        crit = sl.StructureTensorLoss(sigma, rho)

        def fwd():
            return crit(x, gt)

        def fwd_bwd():
            torch.autograd.grad(crit(x, gt), x)
        with torch.no_grad():
            f = replay_us(fwd, a.reps)
        fb = replay_us(fwd_bwd, a.reps)
        out["rows"].append({"path": path, "sigma": sigma, "rho": rho, "radii": list(radii), "fwd_us": round(f, 2),
                            "fwd_bwd_us": round(fb, 2), "bwd_us": round(fb - f, 2)})
    sl.ST_FORCE_GENERAL = False
    out["note"] = "bwd_us = fwd_bwd_us - fwd_us; the backward includes autograd's own launches (the upstream gradient's ones_like)"
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
