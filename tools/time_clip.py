#!/usr/bin/env python3
"""What global gradient-norm clipping and the non-finite guard (SOLVER.G_GRAD_CLIP / D_GRAD_CLIP / SKIP_NONFINITE, csrc/optim.hip:
grad_sumsq_kernel + adam_flat_clip_kernel) cost, in one process per measurement, on the bench's flagship workload (bench.py
build_engine("srgan"): B = 16, 96 px, three discriminator forwards).

    --mode kernels    the optimizer step at the generator's and at the discriminator's size, replayed back to back from a hipGraph:
                      adam_flat, grad_sumsq alone, and grad_sumsq + adam_flat_clip (what FlatAdam.step() launches with the feature
                      on); us per pass
    --mode step       wall time of the whole captured iteration with --clip MAX_NORM for both networks and the guard on (0 = the
                      feature off): `--warmup` untimed steps, then `--steps` timed ones between device syncs, `--repeats` times; the
                      minimum and the median in ms

Prints one JSON line.  Each GPU step under its own time limit, chained:

    timeout -k 10 120 python tools/time_clip.py --mode kernels && \\
    timeout -k 10 240 python tools/time_clip.py --mode step --clip 0 && \\
    timeout -k 10 240 python tools/time_clip.py --mode step --clip 1e30
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "srgan-st_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from time_ema import replay_us  # noqa: E402


def kernels():
    from srganst import ops
    from srganst.config import Config
    from srganst.model import Discriminator, Generator
    from srganst.optim import norm_jobs
    torch.manual_seed(0)
    dev = torch.device("cuda")
    out = {"mode": "kernels", "device": torch.cuda.get_device_name(0)}
    a = (0.9, 0.999, 1e-4, 0.0)
    for name, net in (("G", Generator(Config())), ("D", Discriminator(Config()))):
        params = list(net.parameters())
        offs, n = ops.flat_layout(params)
        jobs = ops.NormJobs(norm_jobs(offs, [p.numel() for p in params]), dev)
        p, g = torch.randn(n, device=dev) * 0.05, torch.randn(n, device=dev) * 1e-3
        m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        lr, steps = torch.tensor(1e-4, device=dev), torch.zeros(len(offs), device=dev)
        partials = torch.zeros(jobs.njobs, device=dev, dtype=torch.float64)
        rec = torch.zeros(6, device=dev, dtype=torch.float64)

        def clipped():
            ops.grad_sumsq(g, jobs, partials)
            ops.adam_flat_clip(p, g, m, v, None, lr, steps, *a, 0.0, True, partials, jobs.njobs, 1e30, True, rec)
        out[name] = {"floats": n, "jobs": jobs.njobs,
                     "adam_flat_us": round(replay_us(lambda: ops.adam_flat(p, g, m, v, lr, steps, *a)), 2),
                     "grad_sumsq_us": round(replay_us(lambda: ops.grad_sumsq(g, jobs, partials)), 2),
                     "grad_sumsq_then_adam_flat_clip_us": round(replay_us(clipped), 2)}
        del p, g, m, v
    out["note"] = "the adam figures include the one-workgroup tick launch in front of the update"
    return out


def step(clip, steps, warmup, repeats):
    from srganst.config import Config
    from srganst.engine import TrainEngine
    from srganst.loss import MSELoss, StructureTensorLoss
    from srganst.model import Discriminator, Generator
    cfg = Config()                                   # bench.py build_engine("srgan", share_d_sr=False)
    torch.manual_seed(cfg.DATA.SEED)
    D, G = Discriminator(cfg).cuda().train(), Generator(cfg).cuda().train()
    cfg.add_g_criterion("Pixel", MSELoss(), 1.0)
    cfg.add_g_criterion("ST", StructureTensorLoss(), 1.0 / 3.0)
    cfg.SOLVER.D_UPDATE_INTERVAL = 1
    cfg.KERNEL.REUSE_D_SR = False
    cfg.SOLVER.G_GRAD_CLIP = cfg.SOLVER.D_GRAD_CLIP = clip
    cfg.SOLVER.SKIP_NONFINITE = clip > 0
    eng = TrainEngine(cfg, G, D, use_graph=True)
    g = torch.Generator().manual_seed(1)
    gt = torch.randint(0, 256, (16, 3, 96, 96), generator=g, dtype=torch.uint8).float() / 255.0
    lr = torch.round(torch.nn.functional.interpolate(gt, scale_factor=0.25, mode="bicubic", antialias=True, align_corners=False) * 255) / 255
    gt, lr = gt.cuda(), lr.cuda()
    for _ in range(max(warmup, 4)):
        eng.step(gt, lr)
    gt, lr = eng.gt, eng.lr
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            eng.step(gt, lr)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / steps * 1e3)
    out = {"mode": "step", "clip": clip, "guard": clip > 0, "graph_active": eng.graph_active, "steps": steps, "repeats": repeats,
           "step_ms_min": round(min(times), 4), "step_ms_median": round(statistics.median(times), 4), "grad_stats": eng.grad_stats()}
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["kernels", "step"], required=True)
    ap.add_argument("--clip", type=float, default=0.0)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    print(json.dumps(kernels() if a.mode == "kernels" else step(a.clip, a.steps, a.warmup, a.repeats)), flush=True)


if __name__ == "__main__":
    main()
