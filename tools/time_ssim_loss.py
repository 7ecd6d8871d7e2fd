#!/usr/bin/env python3
"""What SSIMLoss (csrc/ssim_loss.hip: one forward and one backward launch) costs next to the same criterion written as fp32 torch
ops on the same GPU (tests/ssim_refs.py: the restatement the kernels are tested against - the yardstick, never an earlier build of
the kernels), in one process: forward and forward + backward at B = 16, 96 px and B = 8, 192 px, both channels, each replayed back
to back from a hipGraph, us per call; achieved GB/s of the algorithmic bytes (read sr and gt, write d(sr)) for the HIP path.

With --engine also the step time of a reduced WarmupEngine (two residual blocks, B = 16, 96 px, hipGraph) with Pixel only and with
Pixel + 0.1 SSIM.

Prints one JSON line.  Under its own time limit:

    timeout -k 10 180 python tools/time_ssim_loss.py --engine
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


def engine_step_us(with_ssim, steps):
    from srganst.config import Config
    from srganst.engine import WarmupEngine
    from srganst.loss import MSELoss, SSIMLoss
    from srganst.model import Generator
    cfg = Config()
    cfg.MODEL.G_N_RCB = 2
    torch.manual_seed(0)
    G = Generator(cfg).cuda().train()
    crits, weights = {"Pixel": MSELoss()}, {"Pixel": 1.0}
    if with_ssim:
        crits["SSIM"], weights["SSIM"] = SSIMLoss(), 0.1
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
    import ssim_refs
    from srganst.loss import SSIMLoss
    out = {"device": torch.cuda.get_device_name(0), "rows": []}
    for B, size in SHAPES:
        g = torch.Generator().manual_seed(1)
        gt = torch.rand(B, 3, size, size, generator=g)
        x = (gt + 0.08 * torch.randn(gt.shape, generator=g)).clamp(0, 1).cuda().requires_grad_(True)
        gt = gt.cuda()
        for channel in ("y", "rgb"):
            crit = SSIMLoss(channel)
            row = {"batch": B, "size": size, "channel": channel}
            for name, fn in (("hip", lambda: crit(x, gt)), ("torch", lambda: ssim_refs.ssim_loss(x, gt, channel))):
                with torch.no_grad():
                    f = replay_us(fn, a.reps)
                fb = replay_us(lambda: torch.autograd.grad(fn(), x), a.reps)
                row[name] = {"fwd_us": round(f, 2), "fwd_bwd_us": round(fb, 2), "bwd_us": round(fb - f, 2)}
            nbytes = 3.0 * x.numel() * 4
            row["hip"]["algorithmic_GBps"] = round(nbytes / (row["hip"]["fwd_bwd_us"] * 1e-6) / 1e9, 1)
            row["hip_not_slower"] = row["hip"]["fwd_bwd_us"] <= row["torch"]["fwd_bwd_us"]
            with torch.no_grad():
                row["loss_hip"], row["loss_torch"] = crit(x, gt).item(), ssim_refs.ssim_loss(x, gt, channel).item()
            out["rows"].append(row)
    if a.engine:
        out["warmup_engine_step_us"] = {"pixel": round(engine_step_us(False, a.engine_steps), 1),
                                        "pixel_ssim": round(engine_step_us(True, a.engine_steps), 1)}
    out["note"] = ("fwd_us is measured under no_grad (the HIP forward then writes no maps); bwd_us = fwd_bwd_us - fwd_us and includes "
                   "autograd's own launches; algorithmic bytes = read sr + gt, write d(sr)")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
