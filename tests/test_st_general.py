"""CPU: the general structure-tensor path (csrc/st_general.hip) as far as it goes without a GPU - the routing query, the workspace
formula of DESIGN.md section 15, the host-side refusals of the three new entry points (checked before any launch, so null /
never-dereferenced pointers are safe here) - and the oracle the GPU tests measure that path against held to the reference's own
loss and gradient at the new radii (tests/golden/st_general.npz, written by tests/golden/make_golden_st_general.py)."""
import ctypes

import numpy as np
import pytest
import torch

from abi_checks import FAKE, ST_MAPS_REFUSALS, st_maps_call, st_maps_refuses
from abi_checks import lib as _lib
from conftest import rel_err

# (sigma, rho) -> radii: the pairs of the GPU tests (tests/test_st_general_gpu.py)
GENERAL = {(0.3, 0.3): (1, 1), (0.35, 0.6): (1, 2), (0.35, 5.0): (1, 20), (0.5, 1.0): (2, 4), (0.7, 1.4): (3, 6), (1.0, 2.0): (4, 8),
           (1.0, 0.6): (4, 2), (1.5, 3.0): (6, 12), (2.0, 1.0): (8, 4), (2.0, 5.0): (8, 20), (2.1, 5.1): (8, 20)}
TILE = {(0.5, 2.0): (2, 8), (1.0, 2.5): (4, 10)}
BEYOND = {(2.2, 2.0): (9, 8), (1.0, 5.2): (4, 21), (1.0, 10.0): (4, 40)}


def _route(sigma, rho):
    lib, r1, r2 = _lib(), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.sst_st_route(sigma, rho, ctypes.byref(r1), ctypes.byref(r2))
    return rc, (r1.value, r2.value), lib.sst_last_error()


# ------------------------------------------------------------------------------------------------ route
@pytest.mark.parametrize("pair", list(GENERAL))
def test_route_general(pair):
    rc, radii, _ = _route(*pair)
    assert rc == 1 and radii == GENERAL[pair], (rc, radii)


@pytest.mark.parametrize("pair", list(TILE))
def test_route_tile_builds(pair):
    rc, radii, _ = _route(*pair)
    assert rc == 0 and radii == TILE[pair], (rc, radii)


@pytest.mark.parametrize("pair", list(BEYOND))
def test_route_refuses_beyond_the_bound_with_the_loss_message_form(pair):
    rc, radii, err = _route(*pair)
    r1, r2 = BEYOND[pair]
    assert rc == -2 and radii == (r1, r2)
    assert err == b"sst_st_route: (sigma,rho)=(%g,%g) -> radii (%d,%d) not built" % (pair[0], pair[1], r1, r2), err


def test_route_argument_checks():
    lib, r = _lib(), ctypes.c_int()
    assert lib.sst_st_route(0.5, 2.0, None, ctypes.byref(r)) == -1 and b"null pointer" in lib.sst_last_error()
    assert lib.sst_st_route(0.5, 2.0, ctypes.byref(r), None) == -1
    for bad in (float("nan"), float("inf")):
        assert lib.sst_st_route(bad, 2.0, ctypes.byref(r), ctypes.byref(r)) == -1 and b"finite" in lib.sst_last_error()
        assert lib.sst_st_route(0.5, bad, ctypes.byref(r), ctypes.byref(r)) == -1


def test_python_route_and_switch(monkeypatch):
    from srganst import loss as sl
    from srganst._abi import HipPathError
    assert sl.ST_FORCE_GENERAL is False                                   # default off
    assert sl.st_route(0.5, 2.0) == (False, (2, 8)) and sl.st_route(1.0, 2.5) == (False, (4, 10))
    assert sl.st_route(1.0, 2.0) == (True, (4, 8)) and sl.st_route(2.1, 5.1) == (True, (8, 20))
    monkeypatch.setattr(sl, "ST_FORCE_GENERAL", True)
    assert sl.st_route(0.5, 2.0) == (True, (2, 8)) and sl.st_route(1.0, 2.5) == (True, (4, 10))
    for pair, (r1, r2) in BEYOND.items():                                 # the switch does not widen the bound
        with pytest.raises(HipPathError, match=rf"radii \({r1},{r2}\) not built"):
            sl.st_route(*pair)


# ------------------------------------------------------------------------------------------------ workspace
@pytest.mark.parametrize("shape", [(16, 96, 96), (2, 33, 31), (1, 768, 1024), (3, 1, 1), (2, 48, 40)])
def test_workspace_formula(shape):
    """scratch 14 N, saved 2 N with N = B H W; partials = B x 32 x 32-tiles, the tile builds' count."""
    lib = _lib()
    B, H, W = shape
    a, b, c, t = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    assert lib.sst_st_general_workspace(B, H, W, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0
    n = B * H * W
    assert (a.value, b.value, c.value) == (14 * n, 2 * n, B * ((H + 31) // 32) * ((W + 31) // 32))
    assert lib.sst_st_loss_workspace(B, H, W, ctypes.byref(t)) == 0 and t.value == c.value
    assert lib.sst_st_maps_workspace(B, H, W, ctypes.byref(t)) == 0 and t.value == c.value


def test_workspace_refusals():
    lib = _lib()
    a, b, c = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, -1), (32768, 8, 8)):
        assert lib.sst_st_general_workspace(*bad, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == -1
        assert b"bad shape" in lib.sst_last_error()
    assert lib.sst_st_general_workspace(1, 8, 8, None, ctypes.byref(b), ctypes.byref(c)) == -1
    assert lib.sst_st_general_workspace(1, 8, 8, ctypes.byref(a), None, ctypes.byref(c)) == -1
    assert lib.sst_st_general_workspace(1, 8, 8, ctypes.byref(a), ctypes.byref(b), None) == -1


# ------------------------------------------------------------------------------------------------ refusals of the entry points
def _fwd(ptrs=(FAKE,) * 8, shape=(2, 40, 40), sigma=1.0, rho=2.0):
    lib = _lib()
    return lib.sst_st_general_fwd(*ptrs, *shape, sigma, rho, 1, None), lib.sst_last_error()


def _bwd(ptrs=(FAKE,) * 4, scale_dev=None, shape=(2, 40, 40), sigma=1.0, rho=2.0):
    lib = _lib()
    return lib.sst_st_general_bwd(*ptrs, scale_dev, 1.0, 0, *shape, sigma, rho, None), lib.sst_last_error()


def _maps(sigma=1.0, rho=2.0, **kw):
    return st_maps_call("sst_st_general_maps", sigma=sigma, rho=rho, **kw)


BAD_SHAPES = [(0, 40, 40), (2, 0, 40), (2, 40, -3), (32768, 40, 40)]


@pytest.mark.parametrize("k", range(8))
def test_fwd_refuses_each_null_pointer(k):
    ptrs = tuple(None if i == k else FAKE for i in range(8))
    rc, err = _fwd(ptrs=ptrs)
    assert rc == -1 and err == b"sst_st_general_fwd: null pointer", (rc, err)


@pytest.mark.parametrize("k", range(4))
def test_bwd_refuses_each_null_pointer(k):
    ptrs = tuple(None if i == k else FAKE for i in range(4))
    rc, err = _bwd(ptrs=ptrs)
    assert rc == -1 and err == b"sst_st_general_bwd: null pointer", (rc, err)


@pytest.mark.parametrize("shape", BAD_SHAPES)
def test_entries_refuse_bad_shapes(shape):
    for rc, err in (_fwd(shape=shape), _bwd(shape=shape), _maps(Sx=FAKE, shape=shape)):
        assert rc == -1 and b"bad shape" in err, (rc, err)


@pytest.mark.parametrize("pair", list(BEYOND))
def test_entries_refuse_radii_beyond_the_bound(pair):
    r1, r2 = BEYOND[pair]
    tail = b": (sigma,rho)=(%g,%g) -> radii (%d,%d) not built" % (pair[0], pair[1], r1, r2)
    for name, (rc, err) in (("sst_st_general_fwd", _fwd(sigma=pair[0], rho=pair[1])),
                            ("sst_st_general_bwd", _bwd(sigma=pair[0], rho=pair[1])),
                            ("sst_st_general_maps", _maps(Sx=FAKE, d=FAKE, sigma=pair[0], rho=pair[1]))):
        assert rc == -2 and err == name.encode() + tail, (rc, err)


@pytest.mark.parametrize("kwargs, message", ST_MAPS_REFUSALS[:1] + [(dict(scratch=None, Sx=FAKE), b"null pointer")] + ST_MAPS_REFUSALS[1:])
def test_maps_host_side_refusals(kwargs, message):
    st_maps_refuses("sst_st_general_maps", dict(sigma=1.0, rho=2.0, **kwargs), message)


def test_the_tile_entries_keep_their_refusals():
    """The pairs the general path adds are still "not built" for sst_st_loss_fwd / sst_st_loss_bwd / sst_st_maps: those entries keep
    their behaviour for every input."""
    lib = _lib()
    rc = lib.sst_st_loss_fwd(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 2, 40, 40, 1.0, 2.0, 1, None)
    assert rc == -2 and lib.sst_last_error() == b"sst_st_loss_fwd: (sigma,rho)=(1,2) -> radii (4,8) not built"
    rc = lib.sst_st_loss_bwd(FAKE, FAKE, FAKE, None, 1.0, 0, 2, 40, 40, 1.0, 2.0, None)
    assert rc == -2 and lib.sst_last_error() == b"sst_st_loss_bwd: (sigma,rho)=(1,2) not built"
    rc = lib.sst_st_maps(FAKE, FAKE, FAKE, None, None, None, None, None, 2, 40, 40, 1.0, 2.0, 1, None)
    assert rc == -2 and lib.sst_last_error() == b"sst_st_maps: (sigma,rho)=(1,2) -> radii (4,8) not built"


def test_python_surface_refuses_on_the_host():
    from srganst import st
    from srganst._abi import HipPathError
    from srganst.loss import StructureTensorLoss
    x = torch.rand(2, 3, 8, 8)
    with pytest.raises(HipPathError, match=r"radii \(9,8\) not built"):
        StructureTensorLoss(2.2, 2.0)(x, x)
    with pytest.raises(HipPathError, match="ROCm device"):
        st.st_distance(x, x, 1.0, 2.0)


# ------------------------------------------------------------------------------------------------ the oracle at the new radii
ST_GENERAL_CASES = ["s03r03", "s035r50", "s10r20", "s15r30_raw", "s20r50", "s20r50_eq", "s10r20_nan"]
T = torch.from_numpy


def _case(g, case):
    p = f"st/{case}/"
    sigma, rho, norm, scale = (float(v) for v in g[p + "params"])
    gt = T(g[p + "gt_u8"]).float() * scale
    x = T(g[p + "x_u8"]).float() * scale if p + "x_u8" in g.files else gt.clone()
    if p + "nan_at" in g.files:
        x[tuple(int(i) for i in g[p + "nan_at"])] = float("nan")
    return x, gt, sigma, rho, bool(norm)


def test_fixture_holds_arrays_only(golden):
    g = golden("st_general")                                     # allow_pickle=False: object arrays would not load
    assert sorted({f.split("/")[1] for f in g.files}) == sorted(ST_GENERAL_CASES)
    for f in g.files:
        assert g[f].dtype.kind in "fui", (f, g[f].dtype)
    for case in ST_GENERAL_CASES:
        assert g[f"st/{case}/gt_u8"].shape == (2, 3, 32, 32) and g[f"st/{case}/gt_u8"].dtype == np.uint8
    radii = {c: tuple(max(int(4.0 * float(np.float32(s)) + 0.5), 1) for s in g[f"st/{c}/params"][:2]) for c in ST_GENERAL_CASES}
    assert radii == {"s03r03": (1, 1), "s035r50": (1, 20), "s10r20": (4, 8), "s15r30_raw": (6, 12), "s20r50": (8, 20),
                     "s20r50_eq": (8, 20), "s10r20_nan": (4, 8)}


@pytest.mark.parametrize("case", ST_GENERAL_CASES)
def test_oracle_reproduces_the_reference_at_the_new_radii(golden, case):
    """test_oracle_golden.test_st_loss_and_grad_params's assertions at the radii only the general path runs: the yardstick of
    tests/test_st_general_gpu.py is the reference's arithmetic there too."""
    from oracle import st as ost
    g = golden("st_general")
    p = f"st/{case}/"
    x, gt, sigma, rho, norm = _case(g, case)
    loss, gx = ost.st_loss_and_grad(x, gt, sigma, rho, norm)
    l64, g64 = ost.st_loss_and_grad(x.double(), gt.double(), sigma, rho, norm)
    ref, ref64 = g[p + "loss"].item(), g[p + "loss64"].item()
    fin = np.unpackbits(g[p + "grad_finite"])[:gx.numel()].reshape(gx.shape).astype(bool)
    assert torch.equal(torch.isfinite(gx), T(fin)), "non-finite gradient pattern differs from the reference's"
    if case.endswith("_nan"):
        assert np.isnan(ref) and np.isnan(ref64) and torch.isnan(loss) and torch.isnan(l64)
        assert torch.equal(torch.isfinite(g64), T(np.isfinite(g[p + "grad64"])))
        assert 0 < int(fin.sum()) < fin.size
        # the other image is untouched by the NaN
        assert rel_err(gx[0], g[p + "grad64"][0]) <= max(3 * rel_err(gx[0], g64[0]), 1e-5)
        assert rel_err(g64[0], g[p + "grad64"][0]) < 1e-5
        return
    assert abs(loss.item() - ref) <= 2e-5 * abs(ref)
    assert rel_err(gx, g[p + "grad64"]) <= max(3 * g[p + "grad_ref_err"].item(), 1e-5)
    assert abs(l64.item() - ref64) < 1e-6 * abs(ref64)
    assert rel_err(g64, g[p + "grad64"]) < 1e-5
