#!/usr/bin/env python3
"""Wall time of tiled whole-image inference (srganst/upscale.py: Upscaler) against the whole-image forward, same process, same
generator (full-size SRResNet generator, 64 ch x 16 blocks, x4, eval mode, random weights), synthetic uint8 images:

    510x339     LR 510 x 339 (a DIV2K image's x1/4): the whole-image forward, then Upscaler.upscale_u8 at tile 128 and 256, each
                with the exact halo (40) and with halo 16; every tiled time over the whole-image time next to the geometric
                overhead (tile / (tile - 2*halo))^2 and to the pixels actually run (windows x th x tw over H x W).  A ratio well
                above them means the tile shapes fall on a slow kernel
    2040x1356   LR 2040 x 1356 (a DIV2K image used as INPUT): what the whole-image forward does at this size (its error, if it
                is refused) and the tiled images/s at tile 256, exact halo

Every case runs `--warmup` untimed calls (first-use costs: weight packing, code objects, allocator), then `--repeats` timed ones
with a device synchronise at both ends; minimum, median and maximum are reported (the spread).  Prints one JSON line.
--profile-case CASE:TILE:HALO runs only that tiled case (two calls) and nothing else: the run to put under
`rocprofv3 --kernel-trace --stats` for the share of tile_gather_kernel / tile_scatter_kernel / canvas_to_u8_kernel.
Run it under a time limit, one process:

    timeout -k 10 600 python tools/time_upscale.py [--repeats N] [--cases 510x339,2040x1356]
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

CASES = {"510x339": (339, 510), "2040x1356": (1356, 2040)}       # LR (H, W)


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return {"min_s": round(min(ts), 5), "median_s": round(statistics.median(ts), 5), "max_s": round(max(ts), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cases", default="510x339,2040x1356")
    ap.add_argument("--profile-case", default=None, help="e.g. 510x339:256:40 = case:tile:halo; only this tiled run")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_upscale: needs a ROCm device; a CPU run measures nothing")
    from srganst.config import Config
    from srganst.model import Generator
    from srganst.upscale import Upscaler, receptive_radius
    cfg = Config()
    torch.manual_seed(0)
    G = Generator(cfg).to(cfg.DEVICE).eval()
    R = receptive_radius(cfg.MODEL.G_N_RCB, cfg.DATA.UPSCALE_FACTOR)
    gen = torch.Generator().manual_seed(0)
    images = {n: torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=gen) for n, (h, w) in CASES.items()}

    if a.profile_case:
        name, tile, halo = a.profile_case.split(":")
        up = Upscaler(G, tile=int(tile), halo=int(halo))
        for _ in range(2):
            up.upscale_u8(images[name])
        torch.cuda.synchronize()
        print(json.dumps({"profiled": a.profile_case, "tiles": len(up.plan(*CASES[name]))}))
        return

    out = {"warmup": a.warmup, "repeats": a.repeats, "torch": torch.__version__, "hip": torch.version.hip,
           "device": torch.cuda.get_device_name(0), "exact_halo": R}
    for name in a.cases.split(","):
        H, W = CASES[name]
        img = images[name]
        x = (img.permute(2, 0, 1).float() / 255.0).unsqueeze(0).contiguous().to(cfg.DEVICE)
        res = {"lr": [H, W]}
        try:
            with torch.no_grad():
                res["whole"] = timed(lambda: G(x), a.warmup, a.repeats)
        except Exception as e:      # noqa: BLE001 - recording what the whole-image path does at this size is the point
            res["whole"] = {"error": f"{type(e).__name__}: {e}"[:300]}
            torch.cuda.synchronize()
        print(f"# {name}: whole {res['whole']}", file=sys.stderr, flush=True)
        combos = [(128, R), (128, 16), (256, R), (256, 16)] if name == "510x339" else [(256, R)]
        for tile, halo in combos:
            up = Upscaler(G, tile=tile, halo=halo)
            r = timed(lambda: up.upscale_u8(img), a.warmup, a.repeats)
            plan = up.plan(H, W)
            r["tiles"] = len(plan)
            r["batch"] = up.batch_for(plan.th, plan.tw)
            r["geometric_overhead"] = round((tile / (tile - 2 * halo)) ** 2, 3)      # of an image much larger than a window
            r["pixel_ratio"] = round(len(plan) * plan.th * plan.tw / (H * W), 3)      # window pixels over image pixels, this image
            r["images_per_s"] = round(1.0 / r["median_s"], 3)
            if "median_s" in res["whole"]:
                r["over_whole"] = round(r["median_s"] / res["whole"]["median_s"], 3)
            res[f"tile{tile}_halo{halo}"] = r
            print(f"# {name}: tile {tile} halo {halo}: {r}", file=sys.stderr, flush=True)
        out[name] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
