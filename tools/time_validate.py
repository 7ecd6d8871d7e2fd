#!/usr/bin/env python3
"""Wall time of ONE validation pass (validate._validate as train() / warmup() call it per epoch) by metric path, same process,
same generator (full-size SRResNet generator, 64 ch x 16 blocks, eval mode, random weights), same images:

    host      DataLoader over the PNG pairs (decode per pass) -> generator -> tensor2img(...).cpu() -> numpy PSNR / SSIM per image
    device    device_data.DeviceTestSet (decoded + copied once, timed separately) -> generator -> sst_image_metrics per image,
              one device-to-host copy per pass   (DATA.VALIDATE_ON_DEVICE)

on two synthetic sets written as PNGs into a temporary directory: "set14" = 14 images of Set14-like mixed sizes, "1024x768" = one
image of that size.  Every path runs one untimed pass first (first-use costs), then `--passes` timed ones (device sync at both
ends of each); the minimum is reported.  Also reports the largest |host - device| of the averages.  Prints one JSON line.
Run it under a time limit, one process:

    timeout -k 10 900 python tools/time_validate.py [--passes N] [--sets set14,1024x768]
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
from torch.utils.data import DataLoader  # noqa: E402

UP = 4
SETS = {          # HR (H, W), multiples of the upscale factor
    "set14": ((480, 500), (576, 720), (512, 512), (288, 352), (360, 248), (276, 276), (512, 512), (512, 512), (360, 584),
              (512, 768), (392, 528), (656, 528), (288, 352), (588, 584)),
    "1024x768": ((768, 1024),),
}


def write_pairs(d, sizes, seed=0):
    """GT: bicubic-upsampled coarse noise + fine noise on the 1/255 grid; LR: its x1/4 bicubic (dataset.py's synthesis)."""
    from PIL import Image
    from srganst.bicubic import Bicubic
    g = torch.Generator().manual_seed(seed)
    os.makedirs(os.path.join(d, "gt"))
    os.makedirs(os.path.join(d, "lr"))
    for i, (h, w) in enumerate(sizes):
        base = torch.rand(1, 3, h // 8, w // 8, generator=g)
        x = torch.nn.functional.interpolate(base, size=(h, w), mode="bicubic", align_corners=False)
        x = torch.round((x + 0.03 * torch.randn(x.shape, generator=g)).clamp(0, 1) * 255) / 255
        lr = torch.round(Bicubic("cpu")(x, scale=1.0 / UP).clamp(0, 1) * 255)
        for sub, t in (("gt", x * 255), ("lr", lr)):
            u8 = t[0].to(torch.uint8).permute(1, 2, 0).numpy()
            Image.fromarray(np.ascontiguousarray(u8)).save(os.path.join(d, sub, f"img_{i:03d}.png"))


def timed_passes(fn, passes):
    fn()                                                   # untimed: first-use costs (weight packing, allocator, file cache)
    best, res = float("inf"), None
    for _ in range(passes):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--sets", default="set14,1024x768")
    a = ap.parse_args()
    from srganst.config import Config
    from srganst.dataset import TestImageDataset
    from srganst.device_data import DeviceTestSet
    from srganst.model import Generator
    from srganst.validate import _validate
    cfg = Config()
    torch.manual_seed(0)
    G = Generator(cfg).to(cfg.DEVICE).eval()
    out = {"passes": a.passes, "torch": torch.__version__, "hip": torch.version.hip, "device": torch.cuda.get_device_name(0)}
    devnull = open(os.devnull, "w")
    for name in a.sets.split(","):
        with tempfile.TemporaryDirectory() as tmp:
            write_pairs(tmp, SETS[name])
            gt_dir, lr_dir = os.path.join(tmp, "gt"), os.path.join(tmp, "lr")
            loader = DataLoader(TestImageDataset(gt_dir, lr_dir), batch_size=1, shuffle=False, num_workers=0, drop_last=False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dset = DeviceTestSet.from_dir(gt_dir, lr_dir, cfg.DEVICE)
            torch.cuda.synchronize()
            upload = time.perf_counter() - t0
            stdout, sys.stdout = sys.stdout, devnull         # _validate prints its result line
            try:
                t_host, r_host = timed_passes(lambda: _validate(G, loader, cfg, on_device=False), a.passes)
                t_dev, r_dev = timed_passes(lambda: _validate(G, dset, cfg, on_device=True), a.passes)
            finally:
                sys.stdout = stdout
        n = len(SETS[name])
        out[name] = {"images": n, "host_s": round(t_host, 4), "device_s": round(t_dev, 4), "host_over_device": round(t_host / t_dev, 1),
                     "host_ms_per_image": round(t_host / n * 1e3, 2), "device_ms_per_image": round(t_dev / n * 1e3, 2),
                     "device_set_build_s": round(upload, 4), "psnr": r_host[0], "ssim": r_host[1],
                     "abs_diff_psnr": abs(r_host[0] - r_dev[0]), "abs_diff_ssim": abs(r_host[1] - r_dev[1])}
        print(f"# {name}: host {t_host:.3f} s, device {t_dev:.4f} s per pass over {n} images", file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
