"""CPU: the degradation stage's C-ABI entries are exported and declared and refuse bad arguments on the host - before any launch, so
no GPU is needed (nothing here passes a complete valid argument set to a launcher)."""
import ctypes

from abi_checks import exported_and_declared, lib as _lib, refused as _refused

NAMES = ("sst_gather_crops_degraded", "sst_degrade", "sst_degrade_tile_cols")


def test_symbols_are_exported_and_declared():
    exported_and_declared(NAMES)
    from srganst import device_data
    assert _lib().sst_degrade_tile_cols() == device_data.DEGRADE_TILE_COLS
    assert repr(device_data.Degradation()) == ("Degradation(blur_sigma=(0.2, 4.0), aniso=True, blur_prob=1, noise_sigma=(0.0, 25.0), "
                                               "noise_prob=1, ksize=21)")


def test_bad_arguments_are_refused_with_a_message():
    lib = _lib()
    buf = (ctypes.c_double * 16)()                     # host memory standing in for device pointers: never dereferenced
    p = ctypes.addressof(buf)
    assert p % 32 == 0 or (p + 16) % 32 == 0
    p32 = p if p % 32 == 0 else p + 16                 # 32-byte aligned

    def crops(deg=p32, K=21, S=96, span=16, oh=24, Ty=16, lr=p, B=16, desc=p32, arena_bytes=1 << 20):
        return lib.sst_gather_crops_degraded(p32, arena_bytes, p, 4, desc, B, S, p, p, lr, p, p, p, p, oh, oh, Ty, Ty, span, deg, K, 1,
                                             None)

    def general(deg=p32, K=21, H=23, W=30, oh=5, ow=7, Ty=16, Tx=16, B=2, x=p):
        return lib.sst_degrade(x, deg, B, H, W, K, 1, p, p, p, p, p, oh, ow, Ty, Tx, None)

    for call, who in ((crops, "sst_gather_crops_degraded"), (general, "sst_degrade")):
        for K in (4, 20, 1, 23, 0, -3, 22):
            _refused(call(K=K), who, f"K = {K}", "odd and in 3..21")
        for off in (4, 8, 16):
            _refused(call(deg=p32 + off), who, "deg must be 32-byte aligned")
    # the half window against the crop / the image: the values are named
    _refused(crops(S=8, K=21, oh=2, span=8), "half window 10", "crop side 8")
    _refused(crops(S=4, K=9, oh=1, span=4), "half window 4", "crop side 4")
    _refused(general(H=9, W=30, oh=2), "half window 10", "30x9")
    _refused(general(H=23, W=10, ow=2), "half window 10", "10x23")
    _refused(general(H=7, W=7, K=15, oh=1, ow=1), "half window 7", "7x7")
    # LDS over budget: a 1024-px crop's plane does not fit, whatever the band height
    _refused(crops(S=1024, oh=256, span=16), "B of LDS needed", "S 1024", "> 64 KiB")
    _refused(general(H=4096, W=4096, oh=512, ow=512, Ty=64, Tx=64), "B of LDS needed", "> 64 KiB")
    # the gather's own refusals
    _refused(crops(lr=None), "lr and deg are not optional")
    _refused(crops(deg=None), "lr and deg are not optional")
    _refused(crops(S=98), "multiple of 4")
    _refused(crops(span=0), "span 0")
    _refused(crops(B=70000), "batch 70000")
    _refused(crops(desc=p32 + 8), "desc must be 16-byte aligned")
    _refused(crops(arena_bytes=1000), "multiples of 16")
    _refused(general(x=None), "null pointer")
    _refused(general(B=0), "batch 0")
    _refused(general(oh=0), "bad LR arguments")
    _refused(general(oh=24), "bad LR arguments")


def test_python_refusals():
    import pytest
    import torch
    from srganst import device_data
    x = torch.zeros(1, 3, 16, 16)
    deg = device_data.Degradation.fixed(1, 1, 0, 0).draw(1)
    with pytest.raises(ValueError, match="scale must be 2, 4 or 8"):
        device_data.degrade(x, deg, 3)
    with pytest.raises(ValueError, match="ROCm device"):
        device_data.degrade(x, deg, 4)
