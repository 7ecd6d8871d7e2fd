#!/usr/bin/env python3
"""What the structure-tensor family costs, in one process at B = 16, 96 px (the training crop), each call replayed back to back
from a hipGraph, us per call:

    tile     StructureTensorLoss forward and forward + backward on the two 32 x 32-tile builds (csrc/st_loss.hip):
             (0.5, 2.0) radii (2, 8) and (1.0, 2.5) radii (4, 10)
    general  the same on the separable path (csrc/st_general.hip) next to the tile build, the yardstick:
             tile (0.5, 2.0) | general (0.5, 2.0) forced (loss.ST_FORCE_GENERAL) | (1.0, 2.0) | (1.5, 3.0) | (2.0, 5.0), the bound
    maps     st.st_maps (csrc/st_maps.hip, csrc/st_general.hip) with want = d only and want = every output, on both routes,
             at the training crop and at 1 x 3 x 768 x 1024 (a validation image); median and min - max over --repeats

Prints one JSON line.  Under its own time limit:

    timeout -k 10 120 python tools/time_st.py general
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "srgan-st_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from time_ema import replay_us  # noqa: E402

ROWS = {"tile": [("tile", 0.5, 2.0), ("tile", 1.0, 2.5)],
        "general": [("tile", 0.5, 2.0), ("general", 0.5, 2.0), ("general", 1.0, 2.0), ("general", 1.5, 3.0), ("general", 2.0, 5.0)],
        "maps": [("tile", 0.5, 2.0), ("tile", 1.0, 2.5), ("general", 0.5, 2.0), ("general", 1.5, 3.0)]}
MAPS_SHAPES = [(16, 96, 96), (1, 768, 1024)]


def images(B, H, W):
    g = torch.Generator().manual_seed(1)
    gt = torch.rand(B, 3, H, W, generator=g)
    return (gt + 0.08 * torch.randn(gt.shape, generator=g)).clamp(0, 1).cuda(), gt.cuda()


def loss_row(sl, x, gt, sigma, rho, reps):
    crit = sl.StructureTensorLoss(sigma, rho)
    with torch.no_grad():
        f = replay_us(lambda: crit(x, gt), reps)
    fb = replay_us(lambda: torch.autograd.grad(crit(x, gt), x), reps)
    return {"fwd_us": round(f, 2), "fwd_bwd_us": round(fb, 2), "bwd_us": round(fb - f, 2)}


def maps_rows(x, gt, sigma, rho, reps, repeats):
    from srganst import st
    samples = {"maps d-only": [], "maps all outputs": []}
    want = {"maps d-only": ("d",), "maps all outputs": st.OUTPUTS}
    for _ in range(repeats):                                          # alternate the variants inside each repeat
        for k in samples:
            samples[k].append(replay_us(lambda: st.st_maps(x, gt, sigma, rho, want=want[k]), reps))
    return [{"shape": list(x.shape), "variant": k, "us_median": round(statistics.median(v), 2), "us_min": round(min(v), 2),
             "us_max": round(max(v), 2)} for k, v in samples.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=list(ROWS))
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=96)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a CPU run says nothing about these times"
    from srganst import loss as sl
    shapes = MAPS_SHAPES if a.what == "maps" else [(a.batch, a.size, a.size)]
    out = {"device": torch.cuda.get_device_name(0), "batch": a.batch, "size": a.size, "rows": []}
    for shape in shapes:
        x, gt = images(*shape)
        x.requires_grad_(a.what != "maps")
        for path, sigma, rho in ROWS[a.what]:
            sl.ST_FORCE_GENERAL = path == "general"
            general, radii = sl.st_route(sigma, rho)
            assert general == (path == "general")
            head = {"path": path, "sigma": sigma, "rho": rho, "radii": list(radii)}
            if a.what == "maps":
                out["rows"] += [{**head, **row} for row in maps_rows(x, gt, sigma, rho, a.reps, a.repeats)]
            else:
                out["rows"].append({**head, **loss_row(sl, x, gt, sigma, rho, a.reps)})
            print(json.dumps(out["rows"][-1]), file=sys.stderr, flush=True)
    sl.ST_FORCE_GENERAL = False
    if a.what != "maps":
        out["note"] = "bwd_us = fwd_bwd_us - fwd_us; the backward includes autograd's own launches (the upstream gradient's ones_like)"
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
