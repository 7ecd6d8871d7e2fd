"""CPU: the focal frequency loss's three C-ABI entries are exported and declared, size their workspace by the header's formulas and
refuse bad arguments on the host - before any launch, so no GPU is needed (nothing here passes a complete valid argument set to a
launcher)."""
import ctypes

import pytest

from abi_checks import exported_and_declared, lib as _lib, refused as _refused

NAMES = ("sst_freq_loss_workspace", "sst_freq_loss_fwd", "sst_freq_loss_bwd")


def test_symbols_are_exported_and_declared():
    exported_and_declared(NAMES)
    from srganst.loss import FocalFrequencyLoss, fusable
    assert repr(FocalFrequencyLoss()) == "FocalFrequencyLoss(alpha=1.0)" and repr(FocalFrequencyLoss(2)) == "FocalFrequencyLoss(alpha=2.0)"
    assert not fusable(FocalFrequencyLoss())


@pytest.mark.parametrize("B, H, W", [(16, 96, 96), (8, 192, 192), (2, 45, 33), (1, 1, 1), (1, 512, 5), (3, 512, 512)])
def test_workspace_sizes(B, H, W):
    saved, scratch, parts = ctypes.c_int64(-1), ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert _lib().sst_freq_loss_workspace(B, H, W, ctypes.byref(saved), ctypes.byref(scratch), ctypes.byref(parts)) == 0
    Wh = W // 2 + 1
    S = B * 3 * H * Wh * 2                               # one complex half spectrum per plane
    assert saved.value == S
    assert scratch.value == 2 * S + B * 3 * (-(-Wh // 32)) * (-(-H // 32))
    assert parts.value == 2 * B * 3 * (-(-(H * Wh) // 1024))


def test_bad_arguments_are_refused_with_a_message():
    lib = _lib()
    n = ctypes.c_int64()
    buf = (ctypes.c_double * 8)()                      # host memory standing in for device pointers: never dereferenced
    p = ctypes.addressof(buf)
    ok = dict(B=2, H=32, W=32)

    def ws(**kw):
        a = {**ok, **kw}
        return lib.sst_freq_loss_workspace(a["B"], a["H"], a["W"], ctypes.byref(n), ctypes.byref(n), ctypes.byref(n))

    def fwd(alpha=1.0, **kw):
        a = {**ok, **kw}
        return lib.sst_freq_loss_fwd(p, p, p, p, p, p, p, a["B"], a["H"], a["W"], alpha, None)

    def bwd(**kw):
        a = {**ok, **kw}
        return lib.sst_freq_loss_bwd(p, p, p, None, 1.0, 0, a["B"], a["H"], a["W"], None)

    for call in (ws, fwd, bwd):
        _refused(call(H=0), "size 0x32 not built")
        _refused(call(W=0), "size 32x0 not built")
        _refused(call(H=513), "size 513x32 not built")
        _refused(call(W=513), "size 32x513 not built")
        _refused(call(H=-4), "not built")
        _refused(call(B=0), "batch")
        _refused(call(B=-1), "batch")
        _refused(call(B=21846), "batch")               # 3 B planes exceed the grid's 65535
    for alpha in (-0.5, float("nan"), float("inf"), -float("inf")):
        _refused(fwd(alpha=alpha), "alpha")
    for k in range(3):
        args = [ctypes.byref(n)] * 3
        args[k] = None
        _refused(lib.sst_freq_loss_workspace(2, 32, 32, *args), "null pointer")
    for k in (0, 1, 2, 4, 5, 6):                       # saved (3) may be null: no gradient wanted
        args = [p] * 7
        args[k] = None
        _refused(lib.sst_freq_loss_fwd(*args, 2, 32, 32, 1.0, None), "null pointer")
    for k in range(3):                                 # scale_dev (3) may be null
        args = [p] * 3
        args[k] = None
        _refused(lib.sst_freq_loss_bwd(*args, None, 1.0, 0, 2, 32, 32, None), "null pointer")
    _refused(lib.sst_freq_loss_fwd(p, p, p, p, p, p + 4, p, 2, 32, 32, 1.0, None), "8-byte aligned")
    _refused(lib.sst_freq_loss_bwd(p + 4, p, p, None, 1.0, 0, 2, 32, 32, None), "8-byte aligned")


def test_constructor_refusals():
    from srganst.loss import FocalFrequencyLoss
    for alpha in (-1.0, -1e-9, float("nan"), float("inf"), "1.0", None, True):
        with pytest.raises(ValueError):
            FocalFrequencyLoss(alpha)
    for alpha in (0, 0.0, 0.5, 1, 2.0):
        crit = FocalFrequencyLoss(alpha)
        assert crit.alpha == float(alpha) and crit._ws == {}
