"""What the conv wrappers of srganst.ops hand to the launch seam, against the table recorded from the commit before the routing was
gathered into one place (tests/golden/launch_routes.json, written by tests/golden/make_golden_launch_routes.py): per call the label,
the entry point, the trace name, the FLOPs, the argument tuple (pointers as null / non-null), the shapes of the returned and of the
keep-alive tensors (statistics rows, partial rows, slab and workspace sizes) and every refusal - with no switch set and under each
switch of the table.  The wrappers run on `meta` tensors with ops._launch replaced by a recorder: no GPU call is made."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN

_spec = importlib.util.spec_from_file_location("make_golden_launch_routes", os.path.join(GOLDEN, "make_golden_launch_routes.py"))
mglr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mglr)


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "launch_routes.json")) as f:
        doc = json.load(f)
    assert doc["shapes"] == mglr.shapes() and set(doc["switches"]) == set(mglr.SWITCHES[1:])
    return doc["shapes"], mglr.expand(doc)


@pytest.mark.parametrize("sw", mglr.SWITCHES, ids=[s or "no-switch" for s in mglr.SWITCHES])
def test_wrappers_reproduce_the_recorded_launches(recorded, sw):
    from srganst import ops
    shape_rows, want = recorded
    with mglr.switched(ops, sw):
        got = mglr.record(ops, shape_rows)
    bad = [(row, case, w[case], g.get(case)) for row, w, g in zip(shape_rows, want[sw], got) for case in w if g.get(case) != w[case]]
    bad += [(row, case, None, g[case]) for row, w, g in zip(shape_rows, want[sw], got) for case in g if case not in w]
    assert not bad, f"{len(bad)} calls differ from the recorded table (shape, case, recorded, now): {bad[:4]}"


def test_the_table_covers_every_route(recorded):
    """The grid reaches each entry point the routes choose between, each refusal, and each switch changes something."""
    _, want = recorded
    entries = {l[1] for rows in want.values() for cells in rows for r in cells.values() for l in r.get("launches", [])}
    assert entries >= {"sst_conv_fwd", "sst_conv_pipe_fwd_grp", "sst_conv_ns_fwd", "sst_conv_dgrad_bwdstats", "sst_conv_s2_dgrad",
                       "sst_conv_s2_dgrad_pipe_bwdstats_grp", "sst_conv_wgrad_grp"}
    assert any(r.get("raises") == "HipPathError" for cells in want[""] for r in cells.values())
    for sw in mglr.SWITCHES[1:]:
        assert want[sw] != want[""], sw
