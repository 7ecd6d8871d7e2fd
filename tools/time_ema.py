#!/usr/bin/env python3
"""What the generator's weight average (SOLVER.G_EMA_DECAY, csrc/optim.hip: adam_flat_ema_kernel) costs, in one process per
measurement, on the bench's flagship workload (bench.py build_engine("srgan"): B = 16, 96 px, three discriminator forwards).

    --mode kernels    the flat Adam pass at the generator's size (flat buffer of ~1.55 M floats), replayed back to back from a
                      hipGraph: adam_flat, adam_flat_ema (fused) and adam_flat followed by ema_flat (split); us per pass
    --mode step       wall time of the whole captured iteration with --ema DECAY (0 = off): `--warmup` untimed steps, then `--steps`
                      timed ones between device syncs, `--repeats` times; the minimum and the median in ms

Prints one JSON line.  Each GPU step under its own time limit, chained:

    timeout -k 10 120 python tools/time_ema.py --mode kernels && \\
    timeout -k 10 240 python tools/time_ema.py --mode step --ema 0 && \\
    timeout -k 10 240 python tools/time_ema.py --mode step --ema 0.999

The kernel inside the captured step, a profiler run of its own per setting (the Adam rows of the kernel statistics):

    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d prof_ema_on -o ema_on -- python tools/time_ema.py --mode step --ema 0.999 --steps 50 --repeats 1
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


def replay_us(fn, reps=200):
    """us per call of fn(), replayed from a hipGraph and bracketed by events on the launch stream (no host gaps)."""
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def kernels():
    from srganst import ops
    from srganst.config import Config
    from srganst.model import Generator
    torch.manual_seed(0)
    G = Generator(Config())
    offs, n = ops.flat_layout(list(G.parameters()))
    dev = "cuda"
    p, g = torch.randn(n, device=dev) * 0.05, torch.randn(n, device=dev) * 1e-3
    m, v, ema = torch.zeros(n, device=dev), torch.zeros(n, device=dev), p.clone()
    lr, steps = torch.tensor(1e-4, device=dev), torch.zeros(len(offs), device=dev)
    a = (0.9, 0.999, 1e-4, 0.0)
    out = {"mode": "kernels", "floats": n, "device": torch.cuda.get_device_name(0)}
    out["adam_flat_us"] = round(replay_us(lambda: ops.adam_flat(p, g, m, v, lr, steps, *a)), 2)
    out["adam_flat_ema_us"] = round(replay_us(lambda: ops.adam_flat_ema(p, g, m, v, ema, lr, steps, *a, 0.999, True)), 2)

    def split():
        ops.adam_flat(p, g, m, v, lr, steps, *a)
        ops.ema_flat(ema, p, steps, 0.999, True)
    out["adam_flat_then_ema_flat_us"] = round(replay_us(split), 2)
    out["note"] = "each figure includes the one-workgroup step-counter tick launch in front of the Adam pass"
    return out


def step(ema, steps, warmup, repeats):
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
    cfg.SOLVER.G_EMA_DECAY = ema
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
    out = {"mode": "step", "ema_decay": ema, "graph_active": eng.graph_active, "steps": steps, "repeats": repeats,
           "step_ms_min": round(min(times), 4), "step_ms_median": round(statistics.median(times), 4)}
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["kernels", "step"], required=True)
    ap.add_argument("--ema", type=float, default=0.0)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    print(json.dumps(kernels() if a.mode == "kernels" else step(a.ema, a.steps, a.warmup, a.repeats)), flush=True)


if __name__ == "__main__":
    main()
