"""Records the launch trace one eager training step leaves in ops.TRACE / ops.TRACE_HBM -> tests/golden/step_trace.json.

Needs the GPU.  Per engine (TrainEngine: srgan with MSE + structure-tensor + adversarial loss; WarmupEngine: srresnet) and per trace
key: the number of launches and their summed FLOPs (TRACE) or algorithmic bytes (TRACE_HBM), taken in the order bench.kernel_roofline
uses - one eager step, tracing on, one more step.  Record it from a checkout of the commit whose trace is to be preserved:

    python tests/golden/make_golden_step_trace.py

tests/test_step_trace_gpu.py replays it against the tree under test.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "srgan-st_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
OUT = os.path.join(HERE, "step_trace.json")

# 96 px crops, B = 8: the batched discriminator pass (2 * 8 images, 64 -> 128 at 48 x 48) has 1,152 units and the generator's second
# up-sampling conv 1,152 (N-split kernel, thresholds 1,024 and 512); its first one (288) stays on the general kernel
B, HR = 8, 96
WORKLOADS = ("srgan", "srresnet")


def step_trace(workload):
    """{"mfma": {key: [launches, FLOPs]}, "hbm": {key: [launches, bytes]}} of one eager step of the workload's engine."""
    import torch
    import bench
    from srganst import ops
    eng, _ = bench.build_engine(workload, torch.device("cuda:0"), use_graph=False, hr=HR)
    gt, lr = bench.synth_batch(B, HR, torch.device("cuda:0"), 1)
    saved = ops.OVERLAP, ops.TRACE, ops.TRACE_HBM
    try:
        ops.OVERLAP = False
        eng.step(gt, lr)
        torch.cuda.synchronize()
        ops.TRACE, ops.TRACE_HBM = {}, {}
        eng.step(gt, lr)
        torch.cuda.synchronize()
        summary = lambda t: {k: [len(calls), sum(f for _, f, _ in calls)] for k, calls in sorted(t.items())}
        return {"mfma": summary(ops.TRACE), "hbm": summary(ops.TRACE_HBM)}
    finally:
        ops.OVERLAP, ops.TRACE, ops.TRACE_HBM = saved
        eng.close()


def main():
    doc = {"B": B, "hr": HR, **{w: step_trace(w) for w in WORKLOADS}}
    with open(sys.argv[1] if len(sys.argv) > 1 else OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
