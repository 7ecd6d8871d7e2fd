"""CPU: sst_rescale is exported and declared, and refuses bad arguments on the host - before any launch, so no GPU is needed (nothing
here passes a complete valid argument set to the launcher)."""
import ctypes

from abi_checks import exported_and_declared, lib as _lib, refused as _refused

NAMES = ("sst_rescale",)


def test_symbol_is_exported_and_declared():
    exported_and_declared(NAMES)


def test_bad_arguments_are_refused_with_a_message():
    lib = _lib()
    buf = (ctypes.c_double * 32)()                     # host memory standing in for device pointers: never dereferenced
    p = ctypes.addressof(buf)
    p32 = (p + 31) & ~31                               # 32-byte aligned
    x, y = p32 + 64, p32 + 128

    def call(x=x, y=y, rows=p32, B=2, h=24, w=24, quantise=1):
        return lib.sst_rescale(x, y, rows, B, h, w, quantise, None)

    for kw in (dict(x=None), dict(y=None), dict(rows=None)):
        _refused(call(**kw), "sst_rescale", "null pointer")
    _refused(call(y=x), "sst_rescale", "y == x", "out of place")
    for B in (0, -1, 65536):
        _refused(call(B=B), "sst_rescale", f"batch {B} outside [1, 65535]")
    for h, w in ((0, 24), (24, 0), (-3, 24), (8193, 24), (24, 8193)):
        _refused(call(h=h, w=w), "sst_rescale", f"image {w}x{h} outside 1..8192")
    for off in (4, 8, 16):
        _refused(call(rows=p32 + off), "sst_rescale", "rows must be 32-byte aligned")
