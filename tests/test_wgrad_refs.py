"""CPU: what tests/test_conv_wgrad_fp64_gpu.py stands on.  `wgrad64` against fp64 autograd of F.conv2d; the launch plans restated in
tests/wgrad_refs.py against the host entries of the built library (kernel name, slab chunks, pending reduce, group support) for every
case and on every shape of tests/golden/selection.json; every case against the branch it was chosen for - a case that stops reaching
its branch after a plan change fails here instead of passing quietly; and the integer data of every case inside the exact range of
fp32.  No GPU call is made."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

import glue_refs as G
import wgrad_refs as R
from conftest import GOLDEN, rel_err

ALL = R.CASES + R.GROUPED
IDS = [c["id"] for c in ALL]


@pytest.fixture(scope="module")
def lib():
    from srganst import _abi
    return _abi.lib()


def set_switch(monkeypatch, switch):
    for k in [k for k in os.environ if k.startswith("SST_") and k != "SST_LIB_PATH"]:
        monkeypatch.delenv(k)
    if switch:
        monkeypatch.setenv(*switch)


# ================================================================================================ 1. the reference
@pytest.mark.parametrize("shape, affine, grp", [((2, 5, 7, 3, 4, 3, 1), False, 0), ((3, 6, 8, 4, 5, 3, 2), True, 0), ((2, 7, 9, 2, 3, 1, 1), True, 0),
                                                ((1, 10, 9, 2, 3, 9, 1), False, 0), ((4, 6, 6, 3, 2, 3, 2), True, 2)],
                         ids=["k3_s1", "k3_s2_affine", "k1_affine", "k9", "k3_s2_groups"])
def test_wgrad64_is_the_autograd_weight_gradient(shape, affine, grp):
    B, H, W, cin, cout, k, s = shape
    gen = torch.Generator().manual_seed(3 + sum(shape))
    ho, wo = R.out_hw(H, W, k, s)
    x, dy = torch.randn(B, H, W, cin, generator=gen), torch.randn(B, ho, wo, cout, generator=gen)
    rows = (B // grp,) if grp else ()
    sc, sh = (torch.rand(*rows, cin, generator=gen) + 0.5, torch.randn(*rows, cin, generator=gen)) if affine else (None, None)
    slope = 0.25 if affine else None
    dw, terms = R.wgrad64(x, dy, k, s, sc, sh, slope, grp)
    xin = x.double().permute(0, 3, 1, 2)
    if affine:
        r = lambda c: c.double().view(-1, cin).repeat_interleave(grp if grp else B, 0).view(B, cin, 1, 1)
        xin = F.leaky_relu(xin * r(sc) + r(sh), slope)
    w = torch.zeros(cout, cin, k, k, dtype=torch.float64, requires_grad=True)
    F.conv2d(xin, w, None, s, k // 2).backward(dy.double().permute(0, 3, 1, 2))
    assert rel_err(dw, w.grad) < 1e-12
    wt = torch.zeros(cout, cin, k, k, dtype=torch.float64, requires_grad=True)
    F.conv2d(xin.abs(), wt, None, s, k // 2).backward(dy.double().abs().permute(0, 3, 1, 2))
    assert rel_err(terms, wt.grad) < 1e-12 and bool((terms >= dw.abs() * (1 - 1e-12)).all())


def test_wgrad64_pads_after_the_activation():
    """A constant shift on a zero input: only the taps that stay inside the image see it."""
    x, dy = torch.zeros(1, 2, 2, 1), torch.ones(1, 2, 2, 1)
    dw, _ = R.wgrad64(x, dy, 3, 1, torch.ones(1), torch.full((1,), 2.0), None)
    assert dw.view(3, 3).tolist() == [[2.0, 4.0, 2.0], [4.0, 8.0, 4.0], [2.0, 4.0, 2.0]]


# ================================================================================================ 2. route and branch of every case
@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_library_routes_the_case_as_the_restated_plan_says(lib, monkeypatch, c):
    set_switch(monkeypatch, c["switch"])
    shp, n = c["shape"], c["njobs"]
    p = R.case_plan(c)
    assert lib.sst_conv_wgrad_kernel_name(*shp, n).decode() == p["name"] == c["name"]
    assert lib.sst_conv_wgrad_chunks2(*shp, n) == p["slab_chunks"]
    if n == 1:
        for sc in (0, 1):
            for act in (R.ACT_NONE, R.ACT_SLOPE):
                assert lib.sst_conv_wgrad_pending_reduce(*shp, sc, act) == R.case_plan(c, bool(sc), act)["pending"], (sc, act)
        B = shp[0]
        for grp in sorted({1, 2, 3, max(1, B // 2), B, c["grp"] or 1}):
            assert lib.sst_conv_wgrad_groups_ok(*shp, grp) == R.groups_ok(*shp, grp, env=R.env_of(c)), grp
        if c["grp"]:
            assert lib.sst_conv_wgrad_groups_ok(*shp, c["grp"]) == 1
            bad = next(g for g in range(2, B) if B % g)
            assert lib.sst_conv_wgrad_groups_ok(*shp, bad) == 0
        if c["affine"]:                                   # the same kernel and chunks with an input affine and activation
            q = R.case_plan(c, True, R.ACT_SLOPE)
            assert (q["name"], q["nchunk"]) == (p["name"], p["nchunk"])
        else:                                             # 3-channel input: an affine leaves the 3-channel kernels
            assert R.case_plan(c, True, R.ACT_SLOPE)["kind"] == "general"


@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_case_reaches_its_branch(c):
    p = R.case_plan(c)
    assert p["name"] == c["name"], (p["name"], c["name"])
    for key, want in c["expect"].items():
        got = p["sub"][key] if key in p["sub"] else p[key]
        assert got == want, f"{c['id']}: {key} = {got}, the case was chosen for {want} ({c['why']})"
    assert c["props"](p), f"{c['id']} no longer reaches: {c['why']}"
    assert p["nchunk"] <= p["slab_chunks"] and p["pending"] in (0, p["nchunk"])


def test_case_list_covers_what_it_names():
    """The branches of the issue that are a property of the list, not of one case."""
    kinds = {}
    for c in R.CASES:
        kinds.setdefault(R.case_plan(c)["name"], []).append(c)
    assert set(kinds) == {R._tile % t for t in ((2, 2, 8), (2, 2, 6), (1, 4, 8), (1, 4, 6))} | {
        "conv_wgrad_band_kernel<7>", "conv_wgrad_band_kernel<10>", "conv_wgrad_kernel<true>", "conv_wgrad_kernel<false>",
        "wgrad_k3c3_mfma_kernel", "wgrad_k3c3_kernel"}
    variants = {R.reduce_variant(R.case_plan(c)["pending"], c["shape"][3]) for c in R.CASES if R.case_plan(c)["pending"]}
    assert variants == {"split", "vector", "scalar"}
    assert {c["shape"][5] for c in R.CASES} == {1, 3, 5, 7, 9}
    p = R.case_plan(R.BY_ID["grouped_tap_rechunk"])
    assert p["nchunk"] == 2 < p["slab_chunks"] == 6 == R.plan(*R.BY_ID["grouped_tap_rechunk"]["shape"])["nchunk"]
    assert R.BY_ID["grouped_band7_40_jobs"]["njobs"] == R.WG_TAB_MAX


# ================================================================================================ 3. the plans on the recorded shapes
SWEEP = ["", "SST_WGRAD_S2=0", "SST_WGRAD_S1T=1", "SST_WGRAD_BAND=0", "SST_WGRAD_BAND=1", "SST_WGRAD_NO_K3C3=1", "SST_WGRAD_NO_K3C3_MFMA=1",
         "SST_WGRAD_TILE_NO_DIRECT=1", "SST_WGRAD_GROUP_WGS=64"]


@pytest.mark.parametrize("sw", SWEEP, ids=[s or "no-switch" for s in SWEEP])
def test_restated_plans_equal_the_library_on_the_recorded_shapes(lib, monkeypatch, sw):
    with open(os.path.join(GOLDEN, "selection.json")) as f:
        shapes = json.load(f)["shapes"]
    switch = tuple(sw.split("=")) if sw else None
    set_switch(monkeypatch, switch)
    env = dict([switch]) if switch else {}
    assert len(shapes) > 100
    bad = []
    for shp in shapes:
        B = shp[0]
        for n in (1, 2, 16):
            p = R.plan(*shp, njobs=n, env=env)
            got = (lib.sst_conv_wgrad_kernel_name(*shp, n).decode(), lib.sst_conv_wgrad_chunks2(*shp, n))
            if got != (p["name"], p["slab_chunks"]):
                bad.append((shp, n, got, (p["name"], p["slab_chunks"])))
        for sc in (0, 1):
            for act in (0, 1):
                got, want = lib.sst_conv_wgrad_pending_reduce(*shp, sc, act), R.plan(*shp, 1, bool(sc), act, False, env)["pending"]
                if got != want:
                    bad.append((shp, "pending", sc, act, got, want))
        g = max(1, B // 2)
        if lib.sst_conv_wgrad_groups_ok(*shp, g) != R.groups_ok(*shp, g, env=env):
            bad.append((shp, "groups_ok", g))
    assert not bad, f"{len(bad)} differences (shape, what, library, restated): {bad[:6]}"


# ================================================================================================ 4. the data
@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_integer_data_stays_exact(c):
    """single_data / grouped_data assert `exact` on the sum of magnitudes of every form; here also: the data is what the rules say."""
    jobs = R.grouped_data(c["id"], True) if c["njobs"] > 1 else [R.single_data(c["id"], True)]
    for d in jobs:
        for key in ("x", "dy", "base"):
            assert d[key].dtype == torch.float32 and bool((d[key] == d[key].round()).all()) and float(d[key].abs().max()) <= 3
        assert set(d["sc"].unique().tolist()) <= {0.5, 1.0, 2.0}
        assert bool((d["sh"] == d["sh"].round()).all()) and 1 <= float(d["sh"].abs().min()) and float(d["sh"].abs().max()) <= 3
        refs = d["refs"] if "refs" in d else {d["form"]: d["ref"]}
        for form, (dw, terms) in refs.items():
            unit = 1.0 if form == "plain" else 0.125
            assert bool(((dw / unit) == (dw / unit).round()).all()), (c["id"], form)
            assert float(terms.max() + 3) / unit < 2 ** 24
    if c["grp"]:
        d = jobs[0]
        rows = d["sc"].shape[0]
        assert rows == c["shape"][0] // c["grp"] and all(bool((d["sh"][i] != d["sh"][j]).all()) for i in range(rows) for j in range(i))


@pytest.mark.parametrize("c", [c for c in ALL if c["affine"]], ids=lambda c: c["id"])
def test_random_data_decides_every_activation_branch(c):
    """The inputs are fp32 values, so fmaf(x, scale, shift) has the sign of the fp64 x * scale + shift: no element is undecided."""
    jobs = R.grouped_data(c["id"], False) if c["njobs"] > 1 else [R.single_data(c["id"], False)]
    for d in jobs:
        x, sc, sh = d["x"].double(), d["sc"], d["sh"]
        if c["grp"]:
            sc, sh = (t.repeat_interleave(c["grp"], 0).view(x.shape[0], 1, 1, -1) for t in (sc, sh))
        z64 = x * sc.double() + sh.double()
        assert G.undecided_signs(x, sc, sh, z64)[1] == 0
