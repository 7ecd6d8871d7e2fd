#!/usr/bin/env python3
"""What a criterion behind the term protocol costs next to the same criterion written as fp32 torch ops on the same GPU (the
restatement its kernels are tested against - the yardstick, never an earlier build of the kernels), in one process: forward and
forward + backward at B = 16, 96 px and B = 8, 192 px, us per call, each replayed back to back from a hipGraph, with the achieved
rate of the HIP path.

    ssim   SSIMLoss (csrc/ssim_loss.hip), both channels, against tests/ssim_refs.py; GB/s of the algorithmic bytes (read sr and
           gt, write d(sr))
    freq   FocalFrequencyLoss (csrc/freq_loss.hip) against tests/freq_refs.py (torch.fft.fft2), which is timed eagerly first and
           then, if the vendor FFT can be captured, from a hipGraph as well (a failed capture is reported, not fatal; it is tried
           last); the FMA rate of the four transform passes (H Wh (2 W + 4 H) FMAs per plane and direction, Wh = W/2 + 1)
    grad   GradientLoss (csrc/grad_loss.hip), both operators and both criteria, against tests/grad_refs.py (two grouped conv2d per
           image, sqrt, autograd's backward); GB/s of the algorithmic bytes (read sr and gt, write d(sr))
    gv     GradientVarianceLoss (csrc/grad_loss.hip) at patch_size 8 against tests/grad_refs.py (gray, two conv2d, unfold, var);
           GB/s of the same algorithmic bytes
    artifact  ArtifactLoss (csrc/artifact_loss.hip) at ksize 7, without and with the reference image, against tests/artifact_refs.py
           (pad, unfold, var); GB/s of the algorithmic bytes (read sr and gt - and ref -, write d(sr))
    bp     BackProjectionLoss x4 (csrc/bp_loss.hip), both criteria, against the tap-gather form of bicubic.Bicubic.forward without
           its rounding and autograd's backward; GB/s of the algorithmic bytes (forward: read sr and gt; backward: write d(sr))

With --engine also the step time of a reduced WarmupEngine (two residual blocks, B = 16, 96 px, hipGraph) with Pixel only and with
Pixel + the criterion at its usual weight.  For `artifact` the steps are: Pixel alone (no average: the launches of a step before the
criterion existed), Pixel with the averaged generator on, Pixel + the unrefined term (the criterion's own launches), and Pixel + the
refined term (which adds the buffer copy and one eval-mode generator forward for the reference).

Prints one JSON line.  Under its own time limit:

    timeout -k 10 240 python tools/time_criterion.py freq --engine
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
BP_SCALE = 4


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


def engine_step_us(extra, steps, ema_decay=0.0):
    """extra: None or (name, criterion, weight) beside Pixel; ema_decay: SOLVER.G_EMA_DECAY."""
    from srganst.config import Config
    from srganst.engine import WarmupEngine
    from srganst.loss import MSELoss
    from srganst.model import Generator
    cfg = Config()
    cfg.MODEL.G_N_RCB = 2
    cfg.SOLVER.G_EMA_DECAY = ema_decay
    torch.manual_seed(0)
    G = Generator(cfg).cuda().train()
    crits, weights = {"Pixel": MSELoss()}, {"Pixel": 1.0}
    if extra:
        crits[extra[0]], weights[extra[0]] = extra[1], extra[2]
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


# ---- the per-criterion table.  variants(x, gt, size) -> [(the row's label, criterion, yardstick(x, gt))]; rate(hip, x, size): the
# extra rate columns of a row's "hip" entry; torch: the yardstick's key and timer; engine: (key of the step time, name, factory, weight)
def _ssim_variants(x, gt, size):
    import ssim_refs
    from srganst.loss import SSIMLoss
    return [({"channel": c}, SSIMLoss(c), lambda x, gt, c=c: ssim_refs.ssim_loss(x, gt, c)) for c in ("y", "rgb")]


def _algorithmic_rate(hip, x, size):
    hip["algorithmic_GBps"] = round(3.0 * x.numel() * 4 / (hip["fwd_bwd_us"] * 1e-6) / 1e9, 1)


def _grad_variants(x, gt, size):
    import grad_refs
    from srganst.loss import GradientLoss
    return [({"operator": o, "criterion": c}, GradientLoss(o, c), lambda x, gt, o=o, c=c: grad_refs.gradient_loss(x, gt, o, c))
            for o in ("central", "sobel") for c in ("l1", "mse")]


def _gv_variants(x, gt, size):
    import grad_refs
    from srganst.loss import GradientVarianceLoss
    return [({"patch_size": 8}, GradientVarianceLoss(8), lambda x, gt: grad_refs.gv_loss(x, gt, 8))]


def _artifact_variants(x, gt, size):
    import artifact_refs
    from srganst.loss import ArtifactLoss
    ref = (gt + 0.08 * torch.randn(gt.shape, generator=torch.Generator().manual_seed(2)).cuda()).clamp(0, 1)
    plain, refined = ArtifactLoss(refine=False), ArtifactLoss()
    return [({"ref": False}, plain, lambda x, gt: artifact_refs.artifact_loss(x, gt)),
            ({"ref": True}, lambda x, gt: refined(x, gt, ref), lambda x, gt: artifact_refs.artifact_loss(x, gt, ref))]


def _artifact_rate(row, x):
    images = 4.0 if row["ref"] else 3.0
    row["hip"]["algorithmic_GBps"] = round(images * x.numel() * 4 / (row["hip"]["fwd_bwd_us"] * 1e-6) / 1e9, 1)


def _artifact_engine_rows():
    """(key, what runs beside Pixel, SOLVER.G_EMA_DECAY) of the steps timed beside the plain Pixel step."""
    from srganst.loss import ArtifactLoss
    return [("pixel_ema", None, 0.999), ("pixel_artifact_unrefined_ema", ("Artifact", ArtifactLoss(refine=False), 1.0), 0.999),
            ("pixel_artifact_ema", ("Artifact", ArtifactLoss(), 1.0), 0.999)]


def _freq_variants(x, gt, size):
    import freq_refs
    from srganst.loss import FocalFrequencyLoss
    return [({"alpha": 1.0}, FocalFrequencyLoss(), freq_refs.freq_loss)]


def _freq_rate(hip, x, size):
    fma = x.shape[0] * 3 * size * (size // 2 + 1) * (2 * size + 4 * size)    # per direction
    hip["fwd_GFMAps"] = round(fma / (hip["fwd_us"] * 1e-6) / 1e9, 1)
    hip["fwd_bwd_GFMAps"] = round(2 * fma / (hip["fwd_bwd_us"] * 1e-6) / 1e9, 1)


def _bp_variants(x, gt, size):
    from srganst.bicubic import Bicubic
    from srganst.loss import BackProjectionLoss
    w0, i0, w1, i1 = Bicubic("cuda").tables(size, size, 1.0 / BP_SCALE, x.device)

    def down(x):
        """Bicubic.forward's host branch on a device tensor, without the rounding."""
        out = torch.sum(x[:, :, i0, :] * w0[None, None, :, :, None], dim=3)
        A = out.permute(0, 1, 3, 2)
        return torch.sum(A[:, :, i1, :] * w1[None, None, :, :, None], dim=3).permute(0, 1, 3, 2)

    def torch_bp(x, gt, criterion):
        with torch.no_grad():
            T = torch.round(255 * down(gt)) / 255
        D = down(x) - T
        return D.abs().mean() if criterion == "l1" else (D * D).mean()
    return [({"criterion": c}, BackProjectionLoss(BP_SCALE, c), lambda x, gt, c=c: torch_bp(x, gt, c)) for c in ("l1", "mse")]


def _bp_rate(hip, x, size):
    nb = x.numel() * 4.0
    hip["fwd_algorithmic_GBps"] = round(2 * nb / (hip["fwd_us"] * 1e-6) / 1e9, 1)
    hip["bwd_algorithmic_GBps"] = round(nb / (max(hip["bwd_us"], 1e-3) * 1e-6) / 1e9, 1)


def _engine(key, name, cls, weight):
    def make():
        from srganst import loss
        return name, getattr(loss, cls)(), weight
    return key, make


NOTE = "fwd_us is measured under no_grad (the HIP forward then writes no %s); bwd_us = fwd_bwd_us - fwd_us and includes autograd's own launches"
CRITERIA = {
    "ssim": dict(variants=_ssim_variants, rate=_algorithmic_rate, torch=("torch", replay_us), clamp=True, engine=_engine("pixel_ssim", "SSIM", "SSIMLoss", 0.1),
                 note=NOTE % "maps" + "; algorithmic bytes = read sr + gt, write d(sr)"),
    "freq": dict(variants=_freq_variants, rate=_freq_rate, torch=("torch_eager", eager_us), clamp=False, capture_last=True,
                 engine=_engine("pixel_frequency", "Frequency", "FocalFrequencyLoss", 1.0),
                 note=NOTE % "spectrum" + "; GFMAps counts the four direct-DFT passes only"),
    "grad": dict(variants=_grad_variants, rate=_algorithmic_rate, torch=("torch", replay_us), clamp=True,
                 engine=_engine("pixel_gradient", "Gradient", "GradientLoss", 0.1),
                 note="fwd_us is measured under no_grad (the HIP forward saves nothing either way); bwd_us = fwd_bwd_us - fwd_us and "
                 "includes autograd's own launches; algorithmic bytes = read sr + gt, write d(sr)"),
    "gv": dict(variants=_gv_variants, rate=_algorithmic_rate, torch=("torch", replay_us), clamp=True,
               engine=_engine("pixel_gv", "GV", "GradientVarianceLoss", 0.1),
               note=NOTE % "per-patch values" + "; algorithmic bytes = read sr + gt, write d(sr)"),
    "artifact": dict(variants=_artifact_variants, rate=lambda hip, x, size: None, row_rate=_artifact_rate, torch=("torch", replay_us), clamp=True,
                     engine_rows=_artifact_engine_rows,
                     note=NOTE % "w map" + "; algorithmic bytes = read sr + gt (+ ref), write d(sr); in warmup_engine_step_us the difference "
                     "pixel_artifact_unrefined_ema - pixel_ema is the criterion's own launches, pixel_artifact_ema - "
                     "pixel_artifact_unrefined_ema the reference: the buffer copy and one eval-mode generator forward"),
    "bp": dict(variants=_bp_variants, rate=_bp_rate, torch=("torch", replay_us), clamp=True, on_grid=True, head={"scale": BP_SCALE},
               engine=_engine("pixel_bp", "BackProjection", "BackProjectionLoss", 0.1),
               note=NOTE % "saved map" + " and, for the HIP path, the saved map's store; algorithmic bytes: forward = read sr + gt, "
               "backward = write d(sr)"),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("criterion", choices=list(CRITERIA))
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--engine", action="store_true")
    ap.add_argument("--engine-steps", type=int, default=100)
    a = ap.parse_args()
    from srganst import _abi
    c = CRITERIA[a.criterion]
    tkey, timer = c["torch"]
    out = {"device": torch.cuda.get_device_name(0), **c.get("head", {}), "rows": []}
    work = []
    for B, size in SHAPES:
        g = torch.Generator().manual_seed(1)
        gt = torch.rand(B, 3, size, size, generator=g)
        if c.get("on_grid"):
            gt = torch.round(255 * gt) / 255
        x = gt + 0.08 * torch.randn(gt.shape, generator=g)
        x = (x.clamp(0, 1) if c["clamp"] else x).cuda().requires_grad_(True)
        gt = gt.cuda()
        for label, crit, ref in c["variants"](x, gt, size):
            row = {"batch": B, "size": size, **label}
            row["hip"] = fwd_and_fwd_bwd(replay_us, lambda: crit(x, gt), x, a.reps)
            row[tkey] = fwd_and_fwd_bwd(timer, lambda: ref(x, gt), x, a.reps)
            c["rate"](row["hip"], x, size)
            if "row_rate" in c:
                c["row_rate"](row, x)
            with torch.no_grad():
                row["loss_hip"], row["loss_torch"] = crit(x, gt).item(), ref(x, gt).item()
            print(json.dumps(row), file=sys.stderr, flush=True)
            out["rows"].append(row)
            work.append((row, lambda ref=ref, x=x, gt=gt: ref(x, gt), x))
    if a.engine and "engine_rows" in c:
        out["warmup_engine_step_us"] = {"pixel": round(engine_step_us(None, a.engine_steps), 1)}
        for key, extra, ema in c["engine_rows"]():
            out["warmup_engine_step_us"][key] = round(engine_step_us(extra, a.engine_steps, ema), 1)
        print(json.dumps(out["warmup_engine_step_us"]), file=sys.stderr, flush=True)
    elif a.engine:
        key, make = c["engine"]
        out["warmup_engine_step_us"] = {"pixel": round(engine_step_us(None, a.engine_steps), 1), key: round(engine_step_us(make(), a.engine_steps), 1)}
        print(json.dumps(out["warmup_engine_step_us"]), file=sys.stderr, flush=True)
    if c.get("capture_last"):     # can the yardstick be captured at all?  A failed capture leaves the runtime's sticky error behind.
        for row, ref, x in work:
            try:
                row["torch_graph"] = fwd_and_fwd_bwd(replay_us, ref, x, a.reps)
            except Exception as e:                             # noqa: BLE001
                row["torch_graph"] = None
                row["torch_graph_error"] = f"{type(e).__name__}: {str(e)[:200]}"
                _abi.lib().sst_clear_error()
                break
    for row in out["rows"]:
        best = min(t["fwd_bwd_us"] for t in (row[tkey], row.get("torch_graph")) if t)
        row["hip_not_slower"] = row["hip"]["fwd_bwd_us"] <= best
    out["note"] = c["note"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
