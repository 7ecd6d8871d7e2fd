"""The launch trace a real training step leaves in ops.TRACE / ops.TRACE_HBM (what bench.py's roofline is built from) against the one
recorded from the commit before the launch routing was gathered into one place (tests/golden/step_trace.json, written by
tests/golden/make_golden_step_trace.py): the same keys, and per key the same number of launches and the same summed FLOPs / bytes,
for an eager TrainEngine step (srgan: MSE + structure-tensor + adversarial) and an eager WarmupEngine step at B = 8, 96 px."""
import importlib.util
import json
import os
import re

import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_golden_step_trace", os.path.join(GOLDEN, "make_golden_step_trace.py"))
mgst = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mgst)


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "step_trace.json")) as f:
        doc = json.load(f)
    assert (doc["B"], doc["hr"]) == (mgst.B, mgst.HR)
    return doc


def test_the_fixture_holds_every_route(recorded):
    """The step reaches the general family, the pipelined kernel in forward and stride-2 data-gradient form, and the N-split kernel."""
    keys = "\n".join(k for w in mgst.WORKLOADS for k in recorded[w]["mfma"])
    for pat in (r"^conv_(fwd|band)_kernel<", r"^conv_pipe_kernel<\d+, \d+, 0>", r"^conv_pipe_kernel<1, \d+, 1>", r"^conv_ns_kernel<"):
        assert re.search(pat, keys, re.M), pat


@pytest.mark.parametrize("workload", mgst.WORKLOADS)
def test_an_eager_step_leaves_the_recorded_trace(recorded, workload):
    got = mgst.step_trace(workload)
    for bound in ("mfma", "hbm"):
        want = recorded[workload][bound]
        assert set(got[bound]) == set(want), (bound, sorted(set(got[bound]) ^ set(want)))
        bad = {k: (want[k], got[bound][k]) for k in want if list(got[bound][k]) != list(want[k])}
        assert not bad, f"{bound}: (launches, summed FLOPs / bytes) differ from the recorded trace (recorded, now): {bad}"
