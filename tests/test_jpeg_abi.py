"""CPU: the JPEG stage's C-ABI entries are exported and declared, sst_jpeg refuses bad arguments on the host - before any launch, so
no GPU is needed (nothing here passes a complete valid argument set to the launcher) - and sst_jpeg_tables is the restatement's rule."""
import ctypes

import numpy as np
import pytest

import jpeg_refs as refs
from abi_checks import exported_and_declared, lib as _lib, refused as _refused

NAMES = ("sst_jpeg", "sst_jpeg_tables")


def test_symbols_are_exported_and_declared():
    exported_and_declared(NAMES)
    from srganst import device_data
    assert device_data.JPEG_CHROMA == refs.MODES


def test_bad_arguments_are_refused_with_a_message():
    lib = _lib()
    buf = (ctypes.c_double * 16)()                     # host memory standing in for device pointers: never dereferenced
    p = ctypes.addressof(buf)
    p32 = p if p % 32 == 0 else p + 16                 # 32-byte aligned
    assert p32 % 32 == 0

    def call(lr=p, deg=p32, B=2, h=24, w=24, chroma=1):
        return lib.sst_jpeg(lr, deg, B, h, w, chroma, None)

    _refused(call(lr=None), "sst_jpeg", "null pointer")
    _refused(call(deg=None), "sst_jpeg", "null pointer")
    for B in (0, -1, 65536):
        _refused(call(B=B), "sst_jpeg", f"batch {B} outside [1, 65535]")
    for h, w in ((0, 24), (24, 0), (-3, 24), (8193, 24), (24, 8193)):
        _refused(call(h=h, w=w), "sst_jpeg", f"image {w}x{h} outside 1..8192")
    for chroma in (-1, 2, 420):
        _refused(call(chroma=chroma), "sst_jpeg", f"chroma {chroma} must be 0 (444) or 1 (420)")
    for off in (4, 8, 16):
        _refused(call(deg=p32 + off), "sst_jpeg", "deg must be 32-byte aligned")
    out = (ctypes.c_int * 128)()
    _refused(lib.sst_jpeg_tables(50, None), "sst_jpeg_tables", "null pointer")
    for Q in (0, -1, 101):
        _refused(lib.sst_jpeg_tables(Q, out), "sst_jpeg_tables", f"quality {Q} outside 1..100")


def test_tables_against_the_restatement():
    lib = _lib()
    out = (ctypes.c_int * 128)()
    for Q in range(1, 101):
        assert lib.sst_jpeg_tables(Q, out) == 0
        assert np.array_equal(np.array(out[:]).reshape(2, 8, 8), np.stack(refs.tables(Q))), Q


def test_python_refusals():
    import torch
    from srganst import device_data
    x = torch.zeros(1, 3, 16, 16)
    deg = device_data.Degradation.fixed(1, 1, 0, 0, jpeg=50).draw(1)
    with pytest.raises(ValueError, match="ROCm device"):
        device_data.jpeg(x, deg)
    with pytest.raises(ValueError, match="'444' or '420'"):
        device_data.jpeg(x, deg, chroma="422")
    with pytest.raises(ValueError, match="needs quantise=True"):
        device_data.degrade(x, deg, 4, quantise=False, jpeg_chroma="420")
    with pytest.raises(ValueError, match="'444' or '420'"):
        device_data.degrade(x, deg, 4, jpeg_chroma="411")
