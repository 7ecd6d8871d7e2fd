"""CPU: sst_filter2d is exported and declared, and refuses bad arguments on the host - before any launch, so no GPU is needed (nothing
here passes a complete valid argument set to the launcher)."""
import ctypes

from abi_checks import exported_and_declared, lib as _lib, refused as _refused

NAMES = ("sst_filter2d",)


def test_symbol_is_exported_and_declared():
    exported_and_declared(NAMES)


def test_bad_arguments_are_refused_with_a_message():
    lib = _lib()
    buf = (ctypes.c_double * 32)()                     # host memory standing in for device pointers: never dereferenced
    p = ctypes.addressof(buf)
    p32 = (p + 31) & ~31                               # 32-byte aligned
    x, y, bank = p32 + 64, p32 + 128, p32 + 32

    def call(x=x, y=y, flt=p32, bank=bank, M=4, B=2, h=24, w=24, K=21, quantise=1):
        return lib.sst_filter2d(x, y, flt, bank, M, B, h, w, K, quantise, None)

    for kw in (dict(x=None), dict(y=None), dict(flt=None)):
        _refused(call(**kw), "sst_filter2d", "null pointer")
    _refused(call(y=x), "sst_filter2d", "y == x", "out of place")
    _refused(call(bank=None), "sst_filter2d", "null bank with M = 4")
    _refused(call(M=-1), "sst_filter2d", "bank of -1 kernels")
    for B in (0, -1, 65536):
        _refused(call(B=B), "sst_filter2d", f"batch {B} outside [1, 65535]")
    for h, w in ((0, 24), (24, 0), (-3, 24), (8193, 24), (24, 8193)):
        _refused(call(h=h, w=w), "sst_filter2d", f"image {w}x{h} outside 1..8192")
    for K in (1, 2, 4, 20, 23, -3):
        _refused(call(K=K), "sst_filter2d", f"the window K = {K} must be odd and in 3..21")
    for h, w, K in ((10, 24, 21), (24, 10, 21), (3, 3, 7), (1, 1, 3)):
        _refused(call(h=h, w=w, K=K), "sst_filter2d", f"the half window {K // 2} (K = {K}) must be smaller than the image's shorter side")
    for off in (4, 8, 16):
        _refused(call(flt=p32 + off), "sst_filter2d", "flt must be 32-byte aligned")
    for off in (4, 8):
        _refused(call(bank=bank + off), "sst_filter2d", "bank must be 16-byte aligned")
