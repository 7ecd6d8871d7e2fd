#!/usr/bin/env python3
"""Dev tool: GPU-bound time of a best-buddy patch loss forward+backward at the bench size.
Usage: time_bb.py [bb|gram|pst] [l2|l1]   (loss, matching distance; default bb l2)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "srgan-st_amd"))
import torch
from srganst.loss import BestBuddyLoss, GramLoss, PatchwiseStructureTensorLoss


def timeit(fn, n=30, reps=5):          # us per call, replayed from a captured graph (as tools/ablate_wgrad.py)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(3): fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n): fn()
    g.replay(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    e0.record()
    for _ in range(reps): g.replay()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (n * reps) * 1e3


CLS = {"bb": BestBuddyLoss, "gram": GramLoss, "pst": PatchwiseStructureTensorLoss}
which = sys.argv[1] if len(sys.argv) > 1 else "bb"
dist = sys.argv[2] if len(sys.argv) > 2 else "l2"
B, H = 16, 96
sr = torch.rand(B, 3, H, H, device="cuda", requires_grad=True)
gt = torch.rand(B, 3, H, H, device="cuda")
crit = CLS[which](dist_norm=dist)
def fb():
    sr.grad = None
    crit(sr, gt).backward()
print("%s (dist %s) fwd+bwd B=16 96px: %.1f us" % (CLS[which].__name__, dist, timeit(fb)))
