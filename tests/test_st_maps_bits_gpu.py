"""The bytes of every output of st.st_maps, against the record taken from the commit before the three structure-tensor sources came
to share csrc/st_tile.h (tests/golden/st_maps_bits.json, written by tests/golden/make_golden_st_maps_bits.py): both tile builds, the
general route at two radius pairs and the first tile pair forced down it, each with normalize on and off and with gt=None."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN

_spec = importlib.util.spec_from_file_location("make_golden_st_maps_bits", os.path.join(GOLDEN, "make_golden_st_maps_bits.py"))
mgmb = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mgmb)

with open(os.path.join(GOLDEN, "st_maps_bits.json")) as _f:
    RECORDED = json.load(_f)


def test_the_fixture_holds_the_cases_of_the_generator():
    assert RECORDED["seed"] == mgmb.SEED
    assert list(RECORDED["cases"]) == list(mgmb.cases())
    for rec in RECORDED["cases"].values():
        assert {call: set(outs) for call, outs in rec.items()} == {"normalize": set(mgmb_outputs()), "normalize=False": set(mgmb_outputs()),
                                                                   "gt=None": {"Sx", "Fx"}}


def mgmb_outputs():
    from srganst import st
    return st.OUTPUTS


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(RECORDED["cases"]))
def test_a_case_gives_the_recorded_bits(name):
    got = json.loads(json.dumps(mgmb.cases()[name]()))
    want = RECORDED["cases"][name]
    for call in want:
        print(f"{name} [{call}]: " + ", ".join(f"{k} {'same' if got[call][k] == v else 'DIFFERS'}" for k, v in want[call].items()))
    assert got == want, (name, {c: [k for k in want[c] if got[c].get(k) != want[c][k]] for c in want})
