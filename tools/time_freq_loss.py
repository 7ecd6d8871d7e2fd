#!/usr/bin/env python3
"""What FocalFrequencyLoss (csrc/freq_loss.hip: three forward and two backward launches) costs next to the same criterion written as
fp32 torch ops on the same GPU (tests/freq_refs.py: torch.fft.fft2, the restatement the kernels are tested against - the yardstick,
never an earlier build of the kernels), in one process: forward and forward + backward at B = 16, 96 px and B = 8, 192 px, us per
call; the HIP path replayed back to back from a hipGraph, the yardstick timed eagerly first and then, if the vendor FFT can be
captured, from a hipGraph as well (a failed capture is reported, not fatal; it is tried last).  For the HIP path also the achieved
FMA rate of the four transform passes (H Wh (2 W + 4 H) FMAs per plane and direction, Wh = W/2 + 1).

With --engine also the step time of a reduced WarmupEngine (two residual blocks, B = 16, 96 px, hipGraph) with Pixel only and with
Pixel + 1.0 Frequency.

Prints one JSON line.  Under its own time limit:

    timeout -k 10 240 python tools/time_freq_loss.py --engine
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


def eager_us(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def engine_step_us(with_freq, steps):
    from srganst.config import Config
    from srganst.engine import WarmupEngine
    from srganst.loss import FocalFrequencyLoss, MSELoss
    from srganst.model import Generator
    cfg = Config()
    cfg.MODEL.G_N_RCB = 2
    torch.manual_seed(0)
    G = Generator(cfg).cuda().train()
    crits, weights = {"Pixel": MSELoss()}, {"Pixel": 1.0}
    if with_freq:
        crits["Frequency"], weights["Frequency"] = FocalFrequencyLoss(), 1.0
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


def fwd_and_fwd_bwd(timer, fn, x, reps):
    with torch.no_grad():
        f = timer(fn, reps)
    fb = timer(lambda: torch.autograd.grad(fn(), x), reps)
    return {"fwd_us": round(f, 2), "fwd_bwd_us": round(fb, 2), "bwd_us": round(fb - f, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--engine", action="store_true")
    ap.add_argument("--engine-steps", type=int, default=100)
    a = ap.parse_args()
    import freq_refs
    from srganst import _abi
    from srganst.loss import FocalFrequencyLoss
    out = {"device": torch.cuda.get_device_name(0), "rows": []}
    work = []
    for B, size in SHAPES:
        g = torch.Generator().manual_seed(1)
        gt = torch.rand(B, 3, size, size, generator=g)
        x = (gt + 0.08 * torch.randn(gt.shape, generator=g)).cuda().requires_grad_(True)
        gt = gt.cuda()
        crit = FocalFrequencyLoss()
        row = {"batch": B, "size": size, "alpha": 1.0}
        row["hip"] = fwd_and_fwd_bwd(replay_us, lambda: crit(x, gt), x, a.reps)
        ref = lambda x=x, gt=gt: freq_refs.freq_loss(x, gt)    # noqa: E731  (bound now: it is called again after the loop)
        row["torch_eager"] = fwd_and_fwd_bwd(eager_us, ref, x, a.reps)
        wh = size // 2 + 1
        fma = B * 3 * size * wh * (2 * size + 4 * size)    # per direction
        row["hip"]["fwd_GFMAps"] = round(fma / (row["hip"]["fwd_us"] * 1e-6) / 1e9, 1)
        row["hip"]["fwd_bwd_GFMAps"] = round(2 * fma / (row["hip"]["fwd_bwd_us"] * 1e-6) / 1e9, 1)
        with torch.no_grad():
            row["loss_hip"], row["loss_torch"] = crit(x, gt).item(), ref().item()
        print(json.dumps(row), file=sys.stderr, flush=True)
        out["rows"].append(row)
        work.append((row, ref, x))
    if a.engine:
        out["warmup_engine_step_us"] = {"pixel": round(engine_step_us(False, a.engine_steps), 1),
                                        "pixel_frequency": round(engine_step_us(True, a.engine_steps), 1)}
        print(json.dumps(out["warmup_engine_step_us"]), file=sys.stderr, flush=True)
    # last: can the torch.fft composition be captured at all?  A failed capture leaves the runtime's sticky error behind.
    for row, ref, x in work:
        try:
            row["torch_graph"] = fwd_and_fwd_bwd(replay_us, ref, x, a.reps)
        except Exception as e:                             # noqa: BLE001
            row["torch_graph"] = None
            row["torch_graph_error"] = f"{type(e).__name__}: {str(e)[:200]}"
            _abi.lib().sst_clear_error()
            break
    for row in out["rows"]:
        best = min(t["fwd_bwd_us"] for t in (row["torch_eager"], row.get("torch_graph")) if t)
        row["hip_not_slower"] = row["hip"]["fwd_bwd_us"] <= best
    out["note"] = ("fwd_us is measured under no_grad (the HIP forward then writes no spectrum); bwd_us = fwd_bwd_us - fwd_us and "
                   "includes autograd's own launches; GFMAps counts the four direct-DFT passes only")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
