"""CPU: the six C-ABI entries of the gradient-magnitude and gradient-variance criteria are exported and declared, size their
workspaces as include/srganst.h documents and refuse bad arguments on the host - before any launch, so no GPU is needed (nothing
here passes a complete valid argument set to a launcher)."""
import ctypes

import pytest

from abi_checks import exported_and_declared, lib as _lib, refused as _refused

NAMES = ("sst_grad_loss_workspace", "sst_grad_loss_fwd", "sst_grad_loss_bwd", "sst_gv_loss_workspace", "sst_gv_loss_fwd",
         "sst_gv_loss_bwd")


def test_symbols_are_exported_and_declared():
    exported_and_declared(NAMES)
    from srganst.loss import GradientLoss, GradientVarianceLoss
    assert repr(GradientLoss()) == "GradientLoss(operator='central', criterion='l1', eps=1e-06)"
    assert repr(GradientLoss("sobel", "mse", 1e-3)) == "GradientLoss(operator='sobel', criterion='mse', eps=0.001)"
    assert repr(GradientVarianceLoss()) == "GradientVarianceLoss(patch_size=8)"


@pytest.mark.parametrize("B, H, W", [(2, 1, 7), (2, 33, 65), (16, 96, 96), (1, 75, 64), (8, 192, 192), (3, 32, 64)])
def test_grad_workspace_size(B, H, W):
    parts = ctypes.c_int64(-1)
    assert _lib().sst_grad_loss_workspace(B, H, W, ctypes.byref(parts)) == 0
    # one fp64 partial (two floats) per workgroup = per 32 x 32 tile, plane and image
    assert parts.value == 2 * B * 3 * (-(-H // 32)) * (-(-W // 32))


@pytest.mark.parametrize("B, H, W, p", [(2, 19, 43, 8), (1, 31, 34, 3), (2, 8, 8, 8), (1, 75, 64, 5), (1, 64, 40, 32), (1, 9, 5, 2),
                                        (16, 96, 96, 8), (1, 40, 70, 17)])
def test_gv_workspace_sizes(B, H, W, p):
    saved, parts = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert _lib().sst_gv_loss_workspace(B, H, W, p, ctypes.byref(saved), ctypes.byref(parts)) == 0
    ph, pw, n = H // p, W // p, 32 // p
    assert saved.value == 4 * B * ph * pw
    # one fp64 partial per workgroup = per tile of n x n patches that holds a patch, and image
    assert parts.value == 2 * B * (-(-ph // n)) * (-(-pw // n))


def test_bad_arguments_are_refused_with_a_message():
    lib = _lib()
    n = ctypes.c_int64()
    buf = (ctypes.c_double * 8)()                      # host memory standing in for device pointers: never dereferenced
    p = ctypes.addressof(buf)
    ok = dict(B=2, H=32, W=32, op=1, crit=0, eps=1e-6, patch=8)

    def grad_ws(**kw):
        a = {**ok, **kw}
        return lib.sst_grad_loss_workspace(a["B"], a["H"], a["W"], ctypes.byref(n))

    def grad_fwd(**kw):
        a = {**ok, **kw}
        return lib.sst_grad_loss_fwd(p, p, p, p, p, a["B"], a["H"], a["W"], a["op"], a["crit"], a["eps"], None)

    def grad_bwd(**kw):
        a = {**ok, **kw}
        return lib.sst_grad_loss_bwd(p, p, p, None, 1.0, 0, a["B"], a["H"], a["W"], a["op"], a["crit"], a["eps"], None)

    def gv_ws(**kw):
        a = {**ok, **kw}
        return lib.sst_gv_loss_workspace(a["B"], a["H"], a["W"], a["patch"], ctypes.byref(n), ctypes.byref(n))

    def gv_fwd(**kw):
        a = {**ok, **kw}
        return lib.sst_gv_loss_fwd(p, p, p, p, p, p, a["B"], a["H"], a["W"], a["patch"], None)

    def gv_bwd(**kw):
        a = {**ok, **kw}
        return lib.sst_gv_loss_bwd(p, p, p, None, 1.0, 0, a["B"], a["H"], a["W"], a["patch"], None)

    for call in (grad_ws, grad_fwd, grad_bwd):
        _refused(call(B=0), "bad batch")
        _refused(call(B=21846), "bad batch")           # 3 B planes go into the grid's z
        _refused(call(H=0), "bad image size")
        _refused(call(W=-3), "bad image size")
    for call in (grad_fwd, grad_bwd):
        _refused(call(op=2), "op must be")
        _refused(call(op=-1), "op must be")
        _refused(call(crit=2), "crit must be")
        for eps in (0.0, -1e-6, float("nan"), float("inf")):
            _refused(call(eps=eps), "eps must be finite and positive")
    for call in (gv_ws, gv_fwd, gv_bwd):
        _refused(call(B=0), "bad batch")
        _refused(call(patch=1), "patch must be 2..32")
        _refused(call(patch=33), "patch must be 2..32")
        _refused(call(H=7), "below the patch size 8")
        _refused(call(W=7), "below the patch size 8")
        _refused(call(H=0), "below the patch size 8")
    _refused(lib.sst_grad_loss_workspace(2, 32, 32, None), "null pointer")
    _refused(lib.sst_gv_loss_workspace(2, 32, 32, 8, None, ctypes.byref(n)), "null pointer")
    _refused(lib.sst_gv_loss_workspace(2, 32, 32, 8, ctypes.byref(n), None), "null pointer")
    for k in range(5):
        args = [p] * 5
        args[k] = None
        _refused(lib.sst_grad_loss_fwd(*args, 2, 32, 32, 0, 0, 1e-6, None), "sst_grad_loss_fwd: null pointer")
    for k in range(3):                                 # scale_dev (3) may be null
        args = [p] * 3
        args[k] = None
        _refused(lib.sst_grad_loss_bwd(*args, None, 1.0, 0, 2, 32, 32, 0, 0, 1e-6, None), "sst_grad_loss_bwd: null pointer")
    for k in (0, 1, 2, 4, 5):                          # saved (3) may be null: no gradient wanted
        args = [p] * 6
        args[k] = None
        _refused(lib.sst_gv_loss_fwd(*args, 2, 32, 32, 8, None), "sst_gv_loss_fwd: null pointer")
    for k in range(3):                                 # scale_dev (3) may be null
        args = [p] * 3
        args[k] = None
        _refused(lib.sst_gv_loss_bwd(*args, None, 1.0, 0, 2, 32, 32, 8, None), "sst_gv_loss_bwd: null pointer")
    _refused(lib.sst_grad_loss_fwd(p, p, p, p + 4, p, 2, 32, 32, 0, 0, 1e-6, None), "8-byte aligned")
    _refused(lib.sst_gv_loss_fwd(p, p, p, p, p + 4, p, 2, 32, 32, 8, None), "8-byte aligned")


def test_constructor_refusals():
    from srganst.loss import GradientLoss, GradientVarianceLoss
    for kw in ({"operator": "scharr"}, {"criterion": "l2"}, {"eps": 0.0}, {"eps": -1e-6}, {"eps": float("nan")}, {"eps": float("inf")},
               {"eps": "1e-6"}, {"eps": True}):
        with pytest.raises(ValueError):
            GradientLoss(**kw)
    for p in (1, 33, 0, -8, 8.0, "8", True, None):
        with pytest.raises(ValueError):
            GradientVarianceLoss(p)
    crit = GradientLoss("sobel", "mse", eps=1e-4)
    assert (crit.operator, crit.criterion, crit.eps) == ("sobel", "mse", 1e-4) and crit._ws == {}
    assert [GradientVarianceLoss(p).patch_size for p in (2, 17, 32)] == [2, 17, 32] and GradientVarianceLoss()._ws == {}
