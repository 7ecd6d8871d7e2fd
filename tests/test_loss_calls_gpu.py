"""What the criteria ask of the library, against the record taken from the commit before the pixel-space criteria were gathered
behind one term protocol (tests/golden/loss_calls.json, written by tests/golden/make_golden_loss_calls.py): per case the same calls
with the same arguments in the same order, the same loss and weighted values bit for bit, and the same bytes in sr.grad; the
Fourier-domain and the back-projection criteria against the record taken before their reduction epilogue moved into csrc/common.h.
Then, with no fixture: each of the fourteen loss entries is called from exactly one place in the package."""
import importlib.util
import json
import os
import re

import pytest

from conftest import GOLDEN

_spec = importlib.util.spec_from_file_location("make_golden_loss_calls", os.path.join(GOLDEN, "make_golden_loss_calls.py"))
mglc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mglc)

with open(os.path.join(GOLDEN, "loss_calls.json")) as _f:
    RECORDED = json.load(_f)
PACKAGE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "srgan-st_amd", "srganst")
ONE_SITE = [f"sst_{name}_{d}" for name in ("st_loss", "st_pixel_loss", "st_general", "ssim_loss", "freq_loss", "bp_loss", "pixel_loss")
            for d in ("fwd", "bwd")]


def test_the_fixture_holds_the_cases_of_the_generator():
    assert (RECORDED["shape"], RECORDED["seed"]) == ([mglc.B, mglc.H, mglc.W], mglc.SEED)
    assert list(RECORDED["cases"]) == list(mglc.cases())
    entries = {c[0] for recs in RECORDED["cases"].values() for r in recs for c in r["calls"]}
    assert set(ONE_SITE) <= entries, sorted(set(ONE_SITE) - entries)          # every route the rewrite touched is in the record
    assert {"sst_feat_loss_fwd", "sst_feat_loss_bwd", "sst_bb_match_dist", "sst_bbg_match", "sst_bicubic", "sst_weighted_sum"} <= entries


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(RECORDED["cases"]))
def test_a_case_makes_the_recorded_calls_and_bits(name):
    got = json.loads(json.dumps(mglc.cases()[name]()))                       # tuples -> lists, as the record went through JSON
    want = RECORDED["cases"][name]
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        print(f"{name} [{k}]: {len(g['calls'])} calls, loss {g['loss']} (recorded {w['loss']}), grad {g['grad']} (recorded {w['grad']})")
        assert [c[0] for c in g["calls"]] == [c[0] for c in w["calls"]], (name, k)
        for cg, cw in zip(g["calls"], w["calls"]):
            assert cg == cw, (name, k, cg, cw)
        assert g == w, (name, k, {key: (g[key], w[key]) for key in w if g.get(key) != w[key]})


def test_each_loss_entry_has_one_call_site():
    """A host-source check: `.sst_x_fwd` / `.sst_x_bwd` followed by `(` or `,` (called, or handed to a launcher) appears once."""
    sites = {name: [] for name in ONE_SITE}
    for fname in sorted(os.listdir(PACKAGE)):
        if fname.endswith(".py"):
            with open(os.path.join(PACKAGE, fname)) as f:
                for ln, line in enumerate(f, 1):
                    for name in re.findall(r"\.(sst_\w+)\s*[(,]", line):
                        if name in sites:
                            sites[name].append(f"{fname}:{ln}")
    assert all(len(s) == 1 for s in sites.values()), {n: s for n, s in sites.items() if len(s) != 1}
