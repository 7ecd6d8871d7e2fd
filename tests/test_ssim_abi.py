"""CPU: the SSIM criterion's three C-ABI entries are exported and declared, size their workspace as documented and refuse bad
arguments on the host - before any launch, so no GPU is needed (nothing here passes a complete valid argument set to a launcher)."""
import ctypes

import pytest

from abi_checks import exported_and_declared, lib as _lib, refused as _refused

NAMES = ("sst_ssim_loss_workspace", "sst_ssim_loss_fwd", "sst_ssim_loss_bwd")


def test_symbols_are_exported_and_declared():
    exported_and_declared(NAMES)
    from srganst.loss import SSIMLoss
    assert repr(SSIMLoss()) == "SSIMLoss(channel='y', k1=0.01, k2=0.03)"


@pytest.mark.parametrize("B, H, W, planes", [(2, 11, 11, 1), (2, 12, 43, 3), (16, 96, 96, 1), (1, 75, 64, 3), (8, 192, 192, 3),
                                             (3, 42, 43, 1)])
def test_workspace_sizes(B, H, W, planes):
    maps, parts = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert _lib().sst_ssim_loss_workspace(B, H, W, planes, ctypes.byref(maps), ctypes.byref(parts)) == 0
    assert maps.value == B * planes * (H - 10) * (W - 10) * 3
    # one fp64 partial (two floats) per workgroup = per 32 x 32 tile of outputs, plane and image
    assert parts.value == 2 * B * planes * (-(-(H - 10) // 32)) * (-(-(W - 10) // 32))


def test_bad_arguments_are_refused_with_a_message():
    lib = _lib()
    n = ctypes.c_int64()
    buf = (ctypes.c_double * 8)()                      # host memory standing in for device pointers: never dereferenced
    p = ctypes.addressof(buf)
    ok = dict(B=2, H=32, W=32, planes=1)

    def ws(**kw):
        a = {**ok, **kw}
        return lib.sst_ssim_loss_workspace(a["B"], a["H"], a["W"], a["planes"], ctypes.byref(n), ctypes.byref(n))

    def fwd(k1=0.01, k2=0.03, **kw):
        a = {**ok, **kw}
        return lib.sst_ssim_loss_fwd(p, p, p, p, p, p, a["B"], a["H"], a["W"], a["planes"], k1, k2, None)

    def bwd(**kw):
        a = {**ok, **kw}
        return lib.sst_ssim_loss_bwd(p, p, p, p, None, 1.0, 0, a["B"], a["H"], a["W"], a["planes"], None)

    for call in (ws, fwd, bwd):
        _refused(call(H=10), "11-px minimum")
        _refused(call(W=10), "11-px minimum")
        _refused(call(planes=2), "planes")
        _refused(call(B=0), "batch")
    _refused(fwd(k1=0.0), "k1 and k2")
    _refused(fwd(k2=-0.03), "k1 and k2")
    _refused(fwd(k1=float("nan")), "k1 and k2")
    _refused(lib.sst_ssim_loss_workspace(2, 32, 32, 1, None, ctypes.byref(n)), "null pointer")
    _refused(lib.sst_ssim_loss_workspace(2, 32, 32, 1, ctypes.byref(n), None), "null pointer")
    for k in (0, 1, 2, 4, 5):                          # maps (3) may be null: no gradient wanted
        args = [p] * 6
        args[k] = None
        _refused(lib.sst_ssim_loss_fwd(*args, 2, 32, 32, 1, 0.01, 0.03, None), "null pointer")
    for k in range(4):                                 # scale_dev (4) may be null
        args = [p] * 4
        args[k] = None
        _refused(lib.sst_ssim_loss_bwd(*args, None, 1.0, 0, 2, 32, 32, 1, None), "null pointer")


def test_constructor_refusals():
    from srganst.loss import SSIMLoss
    for kw in ({"channel": "ycbcr"}, {"k1": 0.0}, {"k2": -1.0}, {"k1": float("nan")}, {"k2": float("inf")}, {"k1": "0.01"}):
        with pytest.raises(ValueError):
            SSIMLoss(**kw)
    crit = SSIMLoss("rgb", k1=0.02, k2=0.05)
    assert (crit.channel, crit.k1, crit.k2) == ("rgb", 0.02, 0.05) and crit._ws == {}
