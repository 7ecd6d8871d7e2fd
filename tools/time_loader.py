#!/usr/bin/env python3
"""Rate of train() by data path, B = 16, 96-px crops, full-size SRGAN (G 64 ch x 16 blocks, D 64 ch; adversarial + MSE + structure
tensor / 3, D updated every step - bench.py's workload):

    device tensors   the engine stepped on pre-made device tensors (the rate the kernels can take; no loader at all)
    host             train() with the host DataLoader (PIL decode + CPU Bicubic in one worker, pinned H2D copy)
    host+lr_dev      the same with KERNEL.LR_ON_DEVICE (the LR made on the GPU from the copied GT batch)
    on_device        train() with DATA.ON_DEVICE (device-resident uint8 set, one sst_gather_batch launch per batch)

M synthetic crops on the 1/255 grid are written as PNGs into a temporary directory first; train() reads them from there
(DATA.TRAIN_GT_IMAGES_DIR).  A step's time is taken over steps [S0, S0 + S) of one epoch, with a device sync at both ends only.
The one-time decode + upload of the on_device set is timed separately.  Prints one JSON line.

    python tools/time_loader.py [--images M] [--steps S] [--skip S0] [--cases device,host,host_lr,on_device]
    python tools/time_loader.py --gather-only [--iters N]     # N gather launches alone, for a kernel trace:
        rocprofv3 --kernel-trace --stats -d OUT -o gather -- python tools/time_loader.py --gather-only
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "srgan-st_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch.utils.data import Dataset  # noqa: E402

B, HR, UP = 16, 96, 4


def write_crops(d, m, seed=0):
    """m DIV2K-like 96-px crops (bicubic-upsampled coarse noise, as dataset.SyntheticImageDataset 'lowfreq') on the 1/255 grid."""
    from PIL import Image
    g = torch.Generator().manual_seed(seed)
    for i0 in range(0, m, 256):
        n = min(256, m - i0)
        base = torch.rand(n, 3, HR // 8, HR // 8, generator=g)
        x = torch.nn.functional.interpolate(base, size=(HR, HR), mode="bicubic", align_corners=False)
        u8 = torch.round(x.clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1).numpy()
        for j in range(n):
            Image.fromarray(np.ascontiguousarray(u8[j])).save(os.path.join(d, f"crop_{i0 + j:06d}.png"))


class _OnePair(Dataset):
    def __len__(self):
        return 1

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(0)
        return torch.rand(3, HR, HR, generator=g), torch.rand(3, HR // UP, HR // UP, generator=g)


def make_cfg(gt_dir, name):
    from srganst.config import Config
    from srganst.loss import MSELoss, StructureTensorLoss
    cfg = Config()
    cfg.EXP.NAME = name
    cfg.EXP.N_EPOCHS = 1
    cfg.DATA.TRAIN_GT_IMAGES_DIR = gt_dir
    cfg.DATA.BATCH_SIZE = B
    cfg.LOG_TRAIN_PERIOD = 1 << 30            # only batch 0 logs (one sync), like any long run between log steps
    cfg.add_g_criterion("Pixel", MSELoss(), 1.0)
    cfg.add_g_criterion("ST", StructureTensorLoss(), 1.0 / 3.0)
    cfg.SOLVER.D_UPDATE_INTERVAL = 1
    return cfg


class _Window:
    """Wraps TrainEngine.step: device sync + clock when `skip` and `skip + steps` steps have been issued."""

    def __init__(self, skip, steps):
        from srganst.engine import TrainEngine
        self.cls, self.orig = TrainEngine, TrainEngine.step
        self.skip, self.steps, self.n, self.t = skip, steps, 0, []
        win = self

        def step(eng, gt, lr):
            if win.n in (win.skip, win.skip + win.steps):
                torch.cuda.synchronize()
                win.t.append(time.perf_counter())
            win.n += 1
            return win.orig(eng, gt, lr)
        TrainEngine.step = step

    def close(self):
        self.cls.step = self.orig
        return (self.t[1] - self.t[0]) / self.steps if len(self.t) == 2 else float("nan")


def time_train(gt_dir, name, skip, steps, **switches):
    from srganst.train import train
    cfg = make_cfg(gt_dir, name)
    for k, v in switches.items():
        getattr(cfg, k.split(".")[0])[k.split(".")[1]] = v
    w = _Window(skip, steps)
    try:
        train(cfg, test_dataset=_OnePair(), max_steps_per_epoch=skip + steps + 1)
    finally:
        sec = w.close()
    return sec


def time_device_tensors(gt_dir, skip, steps):
    from srganst.engine import TrainEngine
    from srganst.model import Discriminator, Generator
    cfg = make_cfg(gt_dir, "time_loader_dev_tensors")
    torch.manual_seed(cfg.DATA.SEED)
    D, G = Discriminator(cfg).cuda().train(), Generator(cfg).cuda().train()
    eng = TrainEngine(cfg, G, D)
    g = torch.Generator().manual_seed(1)
    gt = (torch.randint(0, 256, (B, 3, HR, HR), generator=g).float() / 255).cuda()
    lr = (torch.randint(0, 256, (B, 3, HR // UP, HR // UP), generator=g).float() / 255).cuda()
    for _ in range(skip):
        eng.step(gt, lr)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.step(gt, lr)
    torch.cuda.synchronize()
    sec = (time.perf_counter() - t0) / steps
    eng.close()
    return sec


def gather_only(iters):
    from srganst.device_data import DeviceImageSet, DeviceLoader
    g = torch.Generator().manual_seed(0)
    dset = DeviceImageSet(torch.randint(0, 256, (4096, HR, HR, 3), generator=g, dtype=torch.uint8).cuda(), UP)
    ld = DeviceLoader(dset, B)
    ld.bind(torch.empty(B, 3, HR, HR, device="cuda"), torch.empty(B, 3, HR // UP, HR // UP, device="cuda"))
    n = 0
    while n < iters:
        for _ in ld:
            n += 1
            if n == iters:
                break
    torch.cuda.synchronize()
    print(json.dumps({"gather_launches": n, "batch": B, "hr": HR}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--skip", type=int, default=20)
    ap.add_argument("--cases", default="device,host,host_lr,on_device")
    ap.add_argument("--gather-only", action="store_true")
    ap.add_argument("--iters", type=int, default=500)
    a = ap.parse_args()
    if a.gather_only:
        return gather_only(a.iters)
    if a.images < (a.skip + a.steps + 1) * B:
        raise SystemExit(f"--images {a.images} < {(a.skip + a.steps + 1) * B}: the timed window must fit into one epoch")
    cases = a.cases.split(",")
    out = {"batch": B, "hr": HR, "images": a.images, "steps": a.steps, "skip": a.skip}
    with tempfile.TemporaryDirectory() as tmp:
        gt_dir = os.path.join(tmp, "train")
        os.makedirs(gt_dir)
        t0 = time.perf_counter()
        write_crops(gt_dir, a.images)
        out["png_write_s"] = round(time.perf_counter() - t0, 2)
        os.chdir(tmp)                                   # train() writes results/<name>/ checkpoints under the working directory
        if "on_device" in cases:
            from srganst.device_data import DeviceImageSet, decode_threads
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s = DeviceImageSet.from_dir(gt_dir, UP, "cuda")
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            out["decode_upload_s"] = round(dt, 3)
            out["decode_upload_img_s"] = round(len(s) / dt, 1)
            out["decode_threads"] = decode_threads()
            out["store_bytes"] = s.store.numel()
            del s
        runs = {
            "device": lambda: time_device_tensors(gt_dir, a.skip, a.steps),
            "host": lambda: time_train(gt_dir, "tl_host", a.skip, a.steps),
            "host_lr": lambda: time_train(gt_dir, "tl_host_lr", a.skip, a.steps, **{"KERNEL.LR_ON_DEVICE": True}),
            "on_device": lambda: time_train(gt_dir, "tl_on_device", a.skip, a.steps, **{"DATA.ON_DEVICE": True}),
        }
        for c in cases:
            sec = runs[c]()
            out[f"{c}_ms_per_step"] = round(sec * 1e3, 3)
            out[f"{c}_img_s"] = round(B / sec, 1)
            print(f"# {c}: {sec * 1e3:.3f} ms/step, {B / sec:.1f} img/s", file=sys.stderr, flush=True)
        if "device" in cases and "on_device" in cases:
            out["on_device_vs_device_tensors"] = round(out["device_ms_per_step"] / out["on_device_ms_per_step"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
