#!/usr/bin/env python3
"""Dev tool: device time of the structure-tensor maps launch (sst_st_maps) beside the loss forward (sst_st_loss_fwd) and beside the
same maps from the torch composition on the device (oracle.st functions on CUDA tensors: ten conv2d launches per image plus
pointwise glue - what the kernel replaces; imported here only, the product never does).

Per shape (16 x 3 x 96 x 96, the training crop, and 1 x 3 x 768 x 1024, a validation image) and per radius build:
  d-only launch | all-outputs launch | sst_st_loss_fwd | torch composition of d | torch composition of all maps
Each figure is microseconds per call from CUDA events around N back-to-back calls (default 300, after a warm-up of every
variant), repeated --repeats times with the variants alternating; median and min - max over the repeats are printed.  The C entry
points are called directly (ctypes) on preallocated buffers, so the events bracket launches, not allocations.
Writes the table to --out as JSON too."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "srgan-st_amd"))
import torch  # noqa: E402

from oracle import st as ost  # noqa: E402
from srganst import _abi  # noqa: E402


def timed(fn, n):
    """us per call: events around n back-to-back calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def features(S):
    t = S[:, 0] + S[:, 1]
    den = t + 1e-12
    return torch.stack((t, (S[:, 0] - S[:, 1]) / den, 2 * S[:, 2] / den), dim=1)


def variants(B, H, W, sigma, rho):
    lib, st = _abi.lib(), _abi.stream_ptr()
    gen = torch.Generator().manual_seed(0)
    gt = torch.rand(B, 3, H, W, generator=gen).cuda()
    x = (gt + 0.05 * torch.randn(B, 3, H, W, generator=gen).cuda()).clamp(0, 1)
    n = ctypes.c_int64()
    _abi.check(lib.sst_st_maps_workspace(B, H, W, ctypes.byref(n)), "sst_st_maps_workspace")
    Sx, Sgt, Fx, Fgt, gS = (torch.empty_like(x) for _ in range(5))
    d = torch.empty(B, H, W, device="cuda")
    tiles, partials = torch.empty(n.value, device="cuda"), torch.empty(n.value, device="cuda")
    loss = torch.empty((), device="cuda")
    counter = torch.zeros(1, device="cuda", dtype=torch.int32)
    p = _abi.ptr

    def d_only():
        _abi.check(lib.sst_st_maps(p(x), p(gt), None, None, None, None, p(d), None, B, H, W, sigma, rho, 1, st), "sst_st_maps")

    def all_outputs():
        _abi.check(lib.sst_st_maps(p(x), p(gt), p(Sx), p(Sgt), p(Fx), p(Fgt), p(d), p(tiles), B, H, W, sigma, rho, 1, st), "sst_st_maps")

    def loss_fwd():
        _abi.check(lib.sst_st_loss_fwd(p(x), p(gt), p(loss), p(gS), p(partials), p(counter), B, H, W, sigma, rho, 1, st), "sst_st_loss_fwd")

    def torch_d():
        with torch.no_grad():
            return ost.st_intermediates(x, gt, sigma, rho, True)["d"]

    def torch_all():
        with torch.no_grad():
            it = ost.st_intermediates(x, gt, sigma, rho, True)
            return it["S1"], it["S2"], features(it["S1"]), features(it["S2"]), it["d"], it["d"].sum(dim=(1, 2))

    # the variants must agree before any of them is timed
    all_outputs()
    ref = torch_all()
    for name, got, want in (("Sx", Sx, ref[0]), ("Sgt", Sgt, ref[1]), ("Fx", Fx, ref[2]), ("Fgt", Fgt, ref[3]), ("d", d, ref[4])):
        err = float((got.double() - want.double()).norm() / want.double().norm())
        assert err < 1e-3, (name, err)
    return {"maps d-only": d_only, "maps all outputs": all_outputs, "loss fwd": loss_fwd, "torch d": torch_d, "torch all maps": torch_all}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a CPU run says nothing about these times"
    assert a.launches >= 200
    rows = []
    for B, H, W in ((16, 96, 96), (1, 768, 1024)):
        for sigma, rho in ((0.5, 2.0), (1.0, 2.5)):
            fns = variants(B, H, W, sigma, rho)
            for fn in fns.values():                                   # warm-up of every variant at this shape
                timed(fn, 20)
            samples = {k: [] for k in fns}
            for _ in range(a.repeats):                                # alternate the variants inside each repeat
                for k, fn in fns.items():
                    samples[k].append(timed(fn, a.launches))
            for k, v in samples.items():
                row = {"shape": [B, 3, H, W], "sigma": sigma, "rho": rho, "variant": k, "us_median": statistics.median(v),
                       "us_min": min(v), "us_max": max(v)}
                rows.append(row)
                print(f"{B}x3x{H}x{W} (sigma {sigma}, rho {rho})  {k:18s} {row['us_median']:10.1f} us   [{row['us_min']:.1f} - {row['us_max']:.1f}]",
                      flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "launches": a.launches, "repeats": a.repeats, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
