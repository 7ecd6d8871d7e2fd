"""CPU: the back-projection criterion's three C-ABI entries are exported and declared, size their workspace as documented and refuse
bad arguments on the host - before any launch, so no GPU is needed (nothing here passes a complete valid argument set to a
launcher) - and the transposed-table builder is the dense adjoint of tests/bp_refs.py."""
import ctypes

import pytest
import torch

import bp_refs as refs
from abi_checks import exported_and_declared, lib as _lib, refused as _refused

NAMES = ("sst_bp_loss_workspace", "sst_bp_loss_fwd", "sst_bp_loss_bwd")


def test_symbols_are_exported_and_declared():
    exported_and_declared(NAMES)
    from srganst.loss import BackProjectionLoss
    assert repr(BackProjectionLoss()) == "BackProjectionLoss(scale=4, criterion='l1', round_target=True)"
    assert repr(BackProjectionLoss(2, "mse", False, target="lr")) == "BackProjectionLoss(scale=2, criterion='mse', round_target=False, target='lr')"


@pytest.mark.parametrize("B, H, W, s", [(16, 96, 96, 4), (1, 13, 1100, 4), (2, 30, 26, 2), (3, 200, 300, 8), (2, 4, 4, 4)])
def test_workspace_sizes(B, H, W, s):
    saved, parts = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert _lib().sst_bp_loss_workspace(B, H, W, s, ctypes.byref(saved), ctypes.byref(parts)) == 0
    oh, ow = H // s, W // s
    assert saved.value == B * 3 * oh * ow
    # one fp64 partial (two floats) per workgroup = per band of 8 LR rows, tile of 32 LR columns (16 at x8) and image plane
    tile = 16 if s == 8 else 32
    assert parts.value == 2 * B * 3 * (-(-oh // 8)) * (-(-ow // tile))


def test_bad_arguments_are_refused_with_a_message():
    lib = _lib()
    n = ctypes.c_int64()
    buf = (ctypes.c_double * 8)()                      # host memory standing in for device pointers: never dereferenced
    p = ctypes.addressof(buf)
    ok = dict(B=2, H=32, W=48, s=4, Ty=16, Tx=16, crit=0, rnd=1, clamp=0, Ny=10, Nx=10)

    def ws(**kw):
        a = {**ok, **kw}
        return lib.sst_bp_loss_workspace(a["B"], a["H"], a["W"], a["s"], ctypes.byref(n), ctypes.byref(n))

    def fwd(gt=p, lr=None, saved=None, per=None, **kw):
        a = {**ok, **kw}
        return lib.sst_bp_loss_fwd(p, gt, lr, p, per, saved, p, p, p, p, p, p, a["B"], a["H"], a["W"], a["s"], a["Ty"], a["Tx"], a["crit"],
                                   a["rnd"], a["clamp"], None)

    def bwd(**kw):
        a = {**ok, **kw}
        return lib.sst_bp_loss_bwd(p, p, p, p, p, p, None, 1.0, 0, a["B"], a["H"], a["W"], a["s"], a["Ny"], a["Nx"], None)

    for call in (ws, fwd, bwd):
        _refused(call(H=3), "48x3", "minimum")         # H < s: the size is named
        _refused(call(W=3), "3x32", "minimum")
        _refused(call(s=8, H=7), "minimum")
        for s in (0, 1, 3, 16, -4):
            _refused(call(s=s), "scale must be 2, 4 or 8")
        _refused(call(B=0), "batch")
    _refused(fwd(gt=p, lr=p), "exactly one of gt and lr", "both")
    _refused(fwd(gt=None, lr=None), "exactly one of gt and lr", "neither")
    _refused(fwd(saved=p, clamp=1), "clamp_sr")
    _refused(fwd(lr=p, gt=None, saved=p, clamp=1), "clamp_sr")
    for crit in (-1, 2):
        _refused(fwd(crit=crit), "criterion")
    _refused(fwd(Ty=0), "taps")
    _refused(fwd(Tx=19), "taps")
    _refused(bwd(Ny=0), "list widths")
    _refused(bwd(Nx=65), "list widths")
    _refused(lib.sst_bp_loss_workspace(2, 32, 32, 4, None, ctypes.byref(n)), "null pointer")
    _refused(lib.sst_bp_loss_workspace(2, 32, 32, 4, ctypes.byref(n), None), "null pointer")
    tail = (2, 32, 48, 4, 16, 16, 0, 1, 0, None)
    for k in (0, 3, 6, 7, 8, 9, 10, 11):               # gt (1) / lr (2), per_image (4) and saved (5) may be null
        args = [p, p, None, p, None, None, p, p, p, p, p, p]
        args[k] = None
        _refused(lib.sst_bp_loss_fwd(*args, *tail), "null pointer")
    for k in range(6):                                 # scale_dev (6) may be null
        args = [p] * 6
        args[k] = None
        _refused(lib.sst_bp_loss_bwd(*args, None, 1.0, 0, 2, 32, 48, 4, 10, 10, None), "null pointer")


def test_constructor_refusals():
    from srganst.loss import BackProjectionLoss
    for kw in ({"scale": 3}, {"scale": 1}, {"scale": 16}, {"scale": 4.0}, {"scale": "4"}, {"scale": True}, {"criterion": "l2"},
               {"criterion": "huber"}, {"criterion": None}, {"target": "hr"}):
        with pytest.raises(ValueError):
            BackProjectionLoss(**kw)
    crit = BackProjectionLoss(8, "mse", round_target=False)
    assert (crit.scale, crit.criterion, crit.round_target, crit.target) == (8, "mse", False, "gt") and crit._ws == {} and crit._tab == {}


@pytest.mark.parametrize("name", list(refs.CASES))
def test_transposed_tables_are_the_dense_adjoint(name):
    """Scattering each list back gives My^T / Mx^T (a merged border weight is rounded to fp32 once: 1e-7); lists are packed, by
    strictly ascending output index, pads are (-1, 0); with the clamped duplicates merged no list is longer than 4 - listed one by
    one a border list would hold 6 / 10 / 18 entries at x2 / x4 / x8."""
    from srganst.bicubic import _contribute
    from srganst.loss import bp_transposed_tables
    _, H, W, s, _ = refs.CASES[name]
    for n, M in zip((H, W), refs.matrices(H, W, s)):
        w, idx = _contribute(n, int(n * (1.0 / s)), 1.0 / s)
        tw, ti = bp_transposed_tables(w, idx, n)
        assert tw.dtype == torch.float32 and ti.dtype == torch.int32 and tw.shape == ti.shape and tw.shape[0] == n
        dense = torch.zeros(n, M.shape[0], dtype=torch.float64)
        for i in range(n):
            k = int((ti[i] >= 0).sum())
            assert k >= 1 and bool((ti[i, k:] == -1).all()) and bool((tw[i, k:] == 0).all())       # every input pixel is read
            assert bool((ti[i, :k] < M.shape[0]).all()) and ti[i, :k].tolist() == sorted(set(ti[i, :k].tolist()))
            dense[i].index_add_(0, ti[i, :k].long(), tw[i, :k].double())
        assert int((ti >= 0).sum()) == int((M != 0).sum())               # one entry per (input, output) pair that meets
        assert (dense - M.t()).abs().max().item() <= 1e-7
        assert tw.shape[1] == min(4, M.shape[0]), tw.shape
        if M.shape[0] >= 8:
            assert int((ti[n // 2] >= 0).sum()) == 4
        border = int((idx[0] == 0).sum())                                # taps of output 0 clamped onto input 0: merged into one
        assert border >= s and ti[0].tolist()[:2] == ([0, 1] if M.shape[0] > 1 else [0])
        assert abs(tw[0, 0].item() - w[0, :border].double().sum().item()) <= 1e-7
