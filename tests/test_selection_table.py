"""The host-side kernel selectors of libsrganst.so against the table recorded from the commit before they were unified
(tests/golden/selection.json, written by tests/golden/make_golden_selection.py): every number - slab chunks, pending reduces, group
support, tile counts - and every kernel name must come out as recorded, with no dev switch set and under each switch of the table.
The only names that may differ are the ones marked "name_corrected" in the fixture: there the recorded name disagreed with the
launcher of the library it was recorded from, and the fixture keeps both.  No GPU call is made."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN

_spec = importlib.util.spec_from_file_location("make_golden_selection", os.path.join(GOLDEN, "make_golden_selection.py"))
mgs = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mgs)


@pytest.fixture(scope="module")
def doc():
    with open(os.path.join(GOLDEN, "selection.json")) as f:
        d = json.load(f)
    assert d["fields"] == mgs.FIELDS and d["shapes"] == mgs.shapes() and set(d["switches"]) == set(mgs.SWITCHES[1:])
    return d


def _expected(doc, sw):
    want = [list(r) for r in mgs.expand(doc)[sw]]
    for m in doc["name_corrected"]:
        if sw in m["switches"]:
            c = mgs.FIELDS.index(m["field"])
            assert m["name_corrected"] is True and c in mgs.NAME_COLS and doc["names"][want[m["row"]][c]] == m["recorded"]
            want[m["row"]][c] = m["name"]
    return want


@pytest.mark.parametrize("sw", mgs.SWITCHES, ids=[s or "no-switch" for s in mgs.SWITCHES])
def test_selectors_reproduce_the_recorded_table(doc, sw, monkeypatch):
    from srganst import _abi
    for k in [k for k in os.environ if k.startswith("SST_") and k != "SST_LIB_PATH"]:
        monkeypatch.delenv(k)
    if sw:
        monkeypatch.setenv(*sw.split("="))
    names = list(doc["names"])
    got = mgs.record(_abi.lib(), doc["shapes"], names)
    want = _expected(doc, sw)
    bad = []
    for shp, w, g in zip(doc["shapes"], want, got):
        for c, (a, b) in enumerate(zip(w, g)):
            if c in mgs.NAME_COLS:
                a, b = a if isinstance(a, str) else names[a], names[b]
            if a != b:
                bad.append((shp, mgs.FIELDS[c], a, b))
    assert not bad, f"{len(bad)} cells differ from the recorded table (shape, field, recorded, library): {bad[:8]}"
    # two invariants of the plan, for every row: a slab sized by chunks2 holds whatever any form of the launch leaves for the reduce,
    # and coefficient groups are taken by the all-taps tile kernel only
    F = mgs.FIELDS.index
    for shp, g in zip(doc["shapes"], got):
        for f in ("pending_s0a0", "pending_s0a1", "pending_s1a0", "pending_s1a1"):
            assert g[F(f)] <= g[F("chunks2_n1")], (shp, f, g[F(f)], g[F("chunks2_n1")])
        assert not g[F("groups_ok")] or names[g[F("wgrad_name")]].startswith("conv_wgrad_tile_kernel"), (shp, names[g[F("wgrad_name")]])


def test_no_number_of_the_table_is_marked_corrected(doc):
    """Corrections are names only, and every one says which recorded name it replaces."""
    for m in doc["name_corrected"]:
        assert mgs.FIELDS.index(m["field"]) in mgs.NAME_COLS and m["recorded"] != m["name"] and m["switches"]
