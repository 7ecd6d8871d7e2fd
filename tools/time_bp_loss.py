#!/usr/bin/env python3
"""What BackProjectionLoss (csrc/bp_loss.hip: one forward and one backward launch) costs next to the same criterion written as fp32
torch ops on the same GPU - the tap-gather form of bicubic.Bicubic.forward without its rounding (index, multiply, sum per axis,
for sr and for gt) and autograd's backward - in one process: forward and forward + backward at B = 16, 96 px and B = 8, 192 px,
x4, both criteria, each replayed back to back from a hipGraph, us per call; achieved GB/s of the algorithmic bytes (forward: read
sr and gt; backward: write d(sr)) for the two HIP kernels.

With --engine also the step time of a reduced WarmupEngine (two residual blocks, B = 16, 96 px, hipGraph) with Pixel only and with
Pixel + 0.1 BackProjection.

Prints one JSON line.  Under its own time limit:

    timeout -k 10 180 python tools/time_bp_loss.py --engine
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "srgan-st_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from time_ema import replay_us  # noqa: E402

SHAPES = [(16, 96), (8, 192)]
SCALE = 4


def torch_down(x, tables):
    """Bicubic.forward's host branch on a device tensor, without the rounding."""
    w0, i0, w1, i1 = tables
    out = torch.sum(x[:, :, i0, :] * w0[None, None, :, :, None], dim=3)
    A = out.permute(0, 1, 3, 2)
    return torch.sum(A[:, :, i1, :] * w1[None, None, :, :, None], dim=3).permute(0, 1, 3, 2)


def torch_bp(x, gt, tables, criterion):
    with torch.no_grad():
        T = torch.round(255 * torch_down(gt, tables)) / 255
    D = torch_down(x, tables) - T
    return D.abs().mean() if criterion == "l1" else (D * D).mean()


def engine_step_us(with_bp, steps):
    from srganst.config import Config
    from srganst.engine import WarmupEngine
    from srganst.loss import BackProjectionLoss, MSELoss
    from srganst.model import Generator
    cfg = Config()
    cfg.MODEL.G_N_RCB = 2
    torch.manual_seed(0)
    G = Generator(cfg).cuda().train()
    crits, weights = {"Pixel": MSELoss()}, {"Pixel": 1.0}
    if with_bp:
        crits["BackProjection"], weights["BackProjection"] = BackProjectionLoss(), 0.1
    eng = WarmupEngine(cfg, G, crits, weights, use_graph=True)
    g = torch.Generator().manual_seed(1)
    gt, lr = torch.rand(16, 3, 96, 96, generator=g).cuda(), torch.rand(16, 3, 24, 24, generator=g).cuda()
    for _ in range(5):
        eng.step(gt, lr)
    torch.cuda.synchronize()
    assert eng.graph_active
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        eng.step(eng.gt, eng.lr)
    e1.record()
    torch.cuda.synchronize()
    eng.close()
    return e0.elapsed_time(e1) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--engine", action="store_true")
    ap.add_argument("--engine-steps", type=int, default=100)
    a = ap.parse_args()
    from srganst.bicubic import Bicubic
    from srganst.loss import BackProjectionLoss
    out = {"device": torch.cuda.get_device_name(0), "scale": SCALE, "rows": []}
    for B, size in SHAPES:
        g = torch.Generator().manual_seed(1)
        gt = torch.round(255 * torch.rand(B, 3, size, size, generator=g)) / 255
        x = (gt + 0.08 * torch.randn(gt.shape, generator=g)).clamp(0, 1).cuda().requires_grad_(True)
        gt = gt.cuda()
        tables = Bicubic("cuda").tables(size, size, 1.0 / SCALE, x.device)
        for criterion in ("l1", "mse"):
            crit = BackProjectionLoss(SCALE, criterion)
            row = {"batch": B, "size": size, "criterion": criterion}
            for name, fn in (("hip", lambda: crit(x, gt)), ("torch", lambda: torch_bp(x, gt, tables, criterion))):
                with torch.no_grad():
                    f = replay_us(fn, a.reps)
                fb = replay_us(lambda: torch.autograd.grad(fn(), x), a.reps)
                row[name] = {"fwd_us": round(f, 2), "fwd_bwd_us": round(fb, 2), "bwd_us": round(fb - f, 2)}
            nb = x.numel() * 4.0
            row["hip"]["fwd_algorithmic_GBps"] = round(2 * nb / (row["hip"]["fwd_us"] * 1e-6) / 1e9, 1)
            row["hip"]["bwd_algorithmic_GBps"] = round(nb / (max(row["hip"]["bwd_us"], 1e-3) * 1e-6) / 1e9, 1)
            row["hip_not_slower"] = row["hip"]["fwd_bwd_us"] <= row["torch"]["fwd_bwd_us"]
            with torch.no_grad():
                row["loss_hip"], row["loss_torch"] = crit(x, gt).item(), torch_bp(x, gt, tables, criterion).item()
            out["rows"].append(row)
    if a.engine:
        out["warmup_engine_step_us"] = {"pixel": round(engine_step_us(False, a.engine_steps), 1),
                                        "pixel_bp": round(engine_step_us(True, a.engine_steps), 1)}
    out["note"] = ("fwd_us is measured under no_grad (the HIP forward then writes no saved map); bwd_us = fwd_bwd_us - fwd_us and "
                   "includes autograd's own launches and, for the HIP path, the saved map's store; algorithmic bytes: forward = read "
                   "sr + gt, backward = write d(sr)")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
