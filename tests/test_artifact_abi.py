"""CPU: the three C-ABI entries of the artifact-map criterion are exported and declared, size their workspaces as include/srganst.h
documents and refuse bad arguments on the host - before any launch, so no GPU is needed (nothing here passes a complete valid
argument set to a launcher)."""
import ctypes

import pytest

from abi_checks import exported_and_declared, lib as _lib, refused as _refused

NAMES = ("sst_artifact_loss_workspace", "sst_artifact_loss_fwd", "sst_artifact_loss_bwd")


def test_symbols_are_exported_and_declared():
    exported_and_declared(NAMES)
    from srganst.loss import ArtifactLoss, fusable
    assert repr(ArtifactLoss()) == "ArtifactLoss(ksize=7, refine=True)"
    assert repr(ArtifactLoss(11, refine=False)) == "ArtifactLoss(ksize=11, refine=False)"
    assert not fusable(ArtifactLoss()) and not fusable(ArtifactLoss(refine=False))
    assert ArtifactLoss().wants_reference and not ArtifactLoss(refine=False).wants_reference


@pytest.mark.parametrize("B, H, W, k", [(1, 4, 4, 7), (2, 33, 65, 7), (1, 75, 64, 7), (2, 19, 43, 3), (2, 19, 43, 11), (16, 96, 96, 7),
                                        (8, 192, 192, 9), (3, 32, 64, 5)])
def test_workspace_sizes(B, H, W, k):
    maps, stats, parts = ctypes.c_int64(-1), ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert _lib().sst_artifact_loss_workspace(B, H, W, k, ctypes.byref(maps), ctypes.byref(stats), ctypes.byref(parts)) == 0
    tiles = B * (-(-H // 32)) * (-(-W // 32))          # one workgroup per 32 x 32 tile and image
    assert maps.value == B * H * W                     # w: one float per pixel
    assert stats.value == 2 * (2 * tiles + B)          # fp64: two sums per workgroup, then the B global weights
    assert parts.value == 2 * tiles                    # one fp64 partial per workgroup


def test_bad_arguments_are_refused_with_a_message():
    lib = _lib()
    n = ctypes.c_int64()
    buf = (ctypes.c_double * 8)()                      # host memory standing in for device pointers: never dereferenced
    p = ctypes.addressof(buf)
    ok = dict(B=2, H=32, W=32, k=7)

    def ws(**kw):
        a = {**ok, **kw}
        return lib.sst_artifact_loss_workspace(a["B"], a["H"], a["W"], a["k"], ctypes.byref(n), ctypes.byref(n), ctypes.byref(n))

    def fwd(**kw):
        a = {**ok, **kw}
        return lib.sst_artifact_loss_fwd(p, p, p, p, p, p, p, p, p, a["B"], a["H"], a["W"], a["k"], None)

    def bwd(**kw):
        a = {**ok, **kw}
        return lib.sst_artifact_loss_bwd(p, p, p, p, None, 1.0, 0, a["B"], a["H"], a["W"], a["k"], None)

    for call in (ws, fwd, bwd):
        _refused(call(B=0), "bad batch")
        _refused(call(B=65536), "bad batch")
        for k in (1, 2, 4, 6, 8, 10, 12, 13, 0, -7):
            _refused(call(k=k), "ksize must be odd, 3..11")
        _refused(call(H=3), "below the 4-px minimum of the reflected 7x7 window")          # H = p
        _refused(call(W=3), "below the 4-px minimum")
        _refused(call(H=5, k=11), "below the 6-px minimum of the reflected 11x11 window")
        _refused(call(H=1, k=3), "below the 2-px minimum")
        _refused(call(H=0), "below the 4-px minimum")
        _refused(call(W=-3), "below the 4-px minimum")
    for k in range(3):
        args = [ctypes.byref(n)] * 3
        args[k] = None
        _refused(lib.sst_artifact_loss_workspace(2, 32, 32, 7, *args), "sst_artifact_loss_workspace: null pointer")
    for k in (0, 1, 3, 5, 6, 7, 8):                    # ref (2) and wmap (4) may be null
        args = [p] * 9
        args[k] = None
        _refused(lib.sst_artifact_loss_fwd(*args, 2, 32, 32, 7, None), "sst_artifact_loss_fwd: null pointer")
    for k in range(4):                                 # scale_dev (4) may be null
        args = [p] * 4
        args[k] = None
        _refused(lib.sst_artifact_loss_bwd(*args, None, 1.0, 0, 2, 32, 32, 7, None), "sst_artifact_loss_bwd: null pointer")
    _refused(lib.sst_artifact_loss_fwd(p, p, p, p, p, p + 4, p, p, p, 2, 32, 32, 7, None), "8-byte aligned")
    _refused(lib.sst_artifact_loss_fwd(p, p, p, p, p, p, p, p + 4, p, 2, 32, 32, 7, None), "8-byte aligned")


def test_constructor_refusals():
    from srganst.loss import ArtifactLoss
    for k in (1, 2, 4, 6, 8, 10, 12, 13, 0, -7, 7.0, "7", True, None):
        with pytest.raises(ValueError):
            ArtifactLoss(k)
    assert [ArtifactLoss(k).ksize for k in (3, 5, 7, 9, 11)] == [3, 5, 7, 9, 11] and ArtifactLoss()._ws == {}


def test_engines_refuse_the_refined_term_without_an_average():
    """The refusal comes from the constructor's host-side check, before the engine touches a device."""
    from srganst import engine
    from srganst.loss import ArtifactLoss
    with pytest.raises(ValueError, match="G_EMA_DECAY"):
        engine._reference_buffers({"Artifact": ArtifactLoss()}, None, None)
    assert engine._reference_buffers({"Artifact": ArtifactLoss(refine=False)}, None, None) is None
    assert engine._reference_buffers({}, None, None) is None
