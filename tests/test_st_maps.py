"""CPU: the structure-tensor maps (csrc/st_maps.hip, srganst/st.py) as far as they go without a GPU - the two C-ABI entry points and
their host-side refusals (checked before any launch, so null / never-dereferenced pointers are safe here), the config switch, and
the oracle the GPU tests measure the maps against (oracle.st.st_intermediates) held to the reference's own S and per-pixel d
(tests/golden/st_maps.npz, written by tests/golden/make_golden_st_maps.py)."""
import ctypes

import numpy as np
import pytest
import torch

from abi_checks import FAKE, ST_MAPS_REFUSALS, st_maps_call, st_maps_refuses
from abi_checks import lib as _lib
from conftest import rel_err


def test_symbols_and_workspace():
    from srganst import _abi
    raw = ctypes.CDLL(_abi.LIB_PATH)
    assert hasattr(raw, "sst_st_maps") and hasattr(raw, "sst_st_maps_workspace")
    lib, n = _lib(), ctypes.c_int64()
    assert lib.sst_st_maps_workspace(16, 96, 96, ctypes.byref(n)) == 0 and n.value == 16 * 9
    assert lib.sst_st_maps_workspace(2, 33, 31, ctypes.byref(n)) == 0 and n.value == 2 * 2 * 1
    assert lib.sst_st_maps_workspace(1, 768, 1024, ctypes.byref(n)) == 0 and n.value == 24 * 32
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, -1)):
        assert lib.sst_st_maps_workspace(*bad, ctypes.byref(n)) != 0 and b"bad shape" in lib.sst_last_error()
    assert lib.sst_st_maps_workspace(1, 8, 8, None) != 0


# the ids are positional: the order of the cases is kept
@pytest.mark.parametrize("kwargs, message", ST_MAPS_REFUSALS[:1] + [
    (dict(Sx=FAKE, shape=(0, 40, 40)), b"bad shape"),
    (dict(Sx=FAKE, shape=(2, 0, 40)), b"bad shape"),
    (dict(Sx=FAKE, shape=(2, 40, -3)), b"bad shape"),
    (dict(Sx=FAKE, shape=(65536, 40, 40)), b"bad shape"),
] + ST_MAPS_REFUSALS[1:5] + [
    (dict(gt=None, Sx=FAKE, Fx=FAKE, tile_sums=FAKE), b"tile_sums cannot be computed without gt"),
] + ST_MAPS_REFUSALS[5:])
def test_host_side_refusals(kwargs, message):
    st_maps_refuses("sst_st_maps", kwargs, message)


def test_unbuilt_radii_are_unsupported_with_the_loss_message_form():
    """sigma 1 / rho 10 (the reference's structure_tensor defaults) -> radii (4, 40): not built, same wording as sst_st_loss_fwd."""
    rc, err = st_maps_call("sst_st_maps", Sx=FAKE, d=FAKE, sigma=1.0, rho=10.0)
    assert rc == -2 and err == b"sst_st_maps: (sigma,rho)=(1,10) -> radii (4,40) not built", (rc, err)
    lib = _lib()
    rc = lib.sst_st_loss_fwd(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 2, 40, 40, 1.0, 10.0, 1, None)
    assert rc == -2 and lib.sst_last_error() == err.replace(b"sst_st_maps", b"sst_st_loss_fwd")


def test_python_surface_refuses_before_the_library():
    """srganst.st checks dtype / rank / channels / device in loss.py's style; none of this needs a device."""
    from srganst import st
    from srganst._abi import HipPathError
    x = torch.rand(2, 3, 8, 8)
    for fn in (st.structure_tensor, st.st_features):
        with pytest.raises(HipPathError, match="ROCm device"):
            fn(x)
    with pytest.raises(HipPathError, match="ROCm device"):
        st.st_distance(x, x)
    with pytest.raises(HipPathError, match="want must name"):
        st.st_maps(x, x, want=("Sx", "nonsense"))
    with pytest.raises(HipPathError, match="want must name"):
        st.st_maps(x, x, want=())
    c2, s2 = torch.tensor([1.0, -1.0, 0.0, 0.0, 0.6]), torch.tensor([0.0, 0.0, 1.0, -1.0, 0.0])
    assert torch.allclose(st.orientation(c2, s2), torch.tensor([0.0, np.pi / 2, np.pi / 4, -np.pi / 4, 0.0]))
    assert torch.allclose(st.coherence(c2, s2), torch.tensor([1.0, 1.0, 1.0, 1.0, 0.6]))


def test_validate_st_is_opt_in():
    from srganst.config import Config
    assert Config().DATA.VALIDATE_ST is False


# ------------------------------------------------------------------------------------------------ the oracle as a yardstick for maps
PARAMS = {"s05r20": (0.5, 2.0), "s10r25": (1.0, 2.5)}


def _case(g, name):
    p = f"maps/{name}/"
    scale, norm = (float(v) for v in g[p + "params"])
    x = torch.from_numpy(g[p + "x_u8"]).float() * scale
    gt = torch.from_numpy(g[p + "gt_u8"]).float() * scale
    return x, gt, bool(norm)


def test_fixture_holds_arrays_only(golden):
    g = golden("st_maps")                                        # allow_pickle=False: object arrays would not load
    assert sorted({f.split("/")[1] for f in g.files}) == ["raw", "unit"]
    for f in g.files:
        assert g[f].dtype.kind in "fu", (f, g[f].dtype)
    for name in ("unit", "raw"):
        assert g[f"maps/{name}/x_u8"].shape == (2, 3, 24, 20) and g[f"maps/{name}/x_u8"].dtype == np.uint8


@pytest.mark.parametrize("tag", list(PARAMS))
@pytest.mark.parametrize("name", ["unit", "raw"])
def test_oracle_reproduces_the_reference_maps(golden, name, tag):
    """S of x, S of gt and the per-pixel d of oracle.st.st_intermediates against the reference's, 1e-6 norm-wise like the existing
    structure-tensor goldens (test_oracle_golden.test_structure_tensor_blocks).  The reference's structure_tensor takes ONE image
    (utils.py:212-216), so the oracle is called one image at a time too: the same conv2d shapes.  (Called on the batch of two, conv2d
    rounds S differently in the last bit - 9e-8 norm-wise, asserted below at 1e-6 as well - and the normalized chain carries that
    into d as 1.8e-5: fp32 conditioning of d in S, not a difference of arithmetic; the d of the batched call from the reference's own
    S is asserted instead, as test_structure_tensor_blocks does.)  Not vacuous: l2 > 1 on at least a tenth of the pixels."""
    from oracle import st as ost
    g = golden("st_maps")
    x, gt, norm = _case(g, name)
    sigma, rho = PARAMS[tag]
    p = f"maps/{name}/{tag}/"
    ref = {k: torch.from_numpy(g[p + k]) for k in ("Sx", "Sgt", "d")}
    its = [ost.st_intermediates(x[b:b + 1], gt[b:b + 1], sigma, rho, norm) for b in range(x.shape[0])]
    it = {k: torch.cat([i[k] for i in its]) for k in ("S1", "S2", "L", "d")}
    assert it["S1"].dtype == torch.float32 and tuple(it["d"].shape) == (2, 24, 20)
    assert float((it["L"][:, 1] > 1).float().mean()) >= 0.1
    assert float(ref["d"].max() - ref["d"].min()) > 0.1 * float(ref["d"].mean())
    e = {k: rel_err(it[k], ref[r]) for k, r in (("S1", "Sx"), ("S2", "Sgt"), ("d", "d"))}
    batched = ost.st_intermediates(x, gt, sigma, rho, norm)
    eb = {k: rel_err(batched[k], ref[r]) for k, r in (("S1", "Sx"), ("S2", "Sgt"), ("d", "d"))}
    eb["d|ref S"] = rel_err(ost.pixel_distance(ref["Sx"], ref["Sgt"], norm), ref["d"])
    print(f"[{name} {tag}] rel err vs the reference: per image {e}, batched {eb}")
    assert e["S1"] < 1e-6 and e["S2"] < 1e-6 and e["d"] < 1e-6, e
    assert eb["S1"] < 1e-6 and eb["S2"] < 1e-6 and eb["d|ref S"] < 1e-6, eb
