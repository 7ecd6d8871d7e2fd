"""CPU: sst_rescale_to and sst_blur are exported and declared, and refuse bad arguments on the host - before any launch, so no GPU is
needed (nothing here passes a complete valid argument set to a launcher)."""
import ctypes

from abi_checks import exported_and_declared, lib as _lib, refused as _refused

NAMES = ("sst_rescale_to", "sst_blur")


def test_symbols_are_exported_and_declared():
    exported_and_declared(NAMES)


def _pointers():
    buf = (ctypes.c_double * 48)()                     # host memory standing in for device pointers: never dereferenced
    p32 = (ctypes.addressof(buf) + 31) & ~31           # 32-byte aligned
    return buf, p32


def test_rescale_to_refuses_bad_arguments_with_a_message(monkeypatch):
    lib = _lib()
    buf, p32 = _pointers()
    x, y = p32 + 64, p32 + 128

    def call(x=x, y=y, rows=p32, B=2, H=96, W=96, h=24, w=24, quantise=1):
        return lib.sst_rescale_to(x, y, rows, B, H, W, h, w, quantise, None)

    for kw in (dict(x=None), dict(y=None), dict(rows=None)):
        _refused(call(**kw), "sst_rescale_to", "null pointer")
    _refused(call(y=x), "sst_rescale_to", "y == x", "out of place")
    for B in (0, -1, 65536):
        _refused(call(B=B), "sst_rescale_to", f"batch {B} outside [1, 65535]")
    for H, W in ((0, 96), (96, 0), (-3, 96), (8193, 96), (96, 8193)):
        _refused(call(H=H, W=W), "sst_rescale_to", f"input image {W}x{H} outside 1..8192")
    for h, w in ((0, 24), (24, 0), (-3, 24), (8193, 24), (24, 8193)):
        _refused(call(h=h, w=w), "sst_rescale_to", f"output image {w}x{h} outside 1..8192")
    for h, w in ((97, 24), (24, 97)):
        _refused(call(h=h, w=w), "sst_rescale_to", f"the output {w}x{h} is larger than the input 96x96")
    for h, w in ((5, 24), (24, 5)):                    # 96 > 16 * 5
        _refused(call(h=h, w=w), "sst_rescale_to", f"the input 96x96 is more than 16 times the output {w}x{h}")
    for off in (4, 8, 16):
        _refused(call(rows=p32 + off), "sst_rescale_to", "rows must be 32-byte aligned")
    # no tile shape that fits: the launcher's own choice always does (1 x 1 at the least: 37 x 37 intermediate pixels at x16), so
    # only a tile forced by the dev switch can ask for more than the budget
    monkeypatch.setenv("SST_RESIZE1_TILE", "32x32")
    _refused(call(), "sst_rescale_to", "B of LDS needed by a 32x32 tile (96x96 -> 24x24) > 64 KiB")
    monkeypatch.delenv("SST_RESIZE1_TILE")


def test_blur_refuses_bad_arguments_with_a_message():
    lib = _lib()
    buf, p32 = _pointers()
    x, y = p32 + 64, p32 + 128

    def call(x=x, deg=p32, y=y, B=2, H=48, W=40, K=21):
        return lib.sst_blur(x, deg, y, B, H, W, K, None)

    for kw in (dict(x=None), dict(y=None), dict(deg=None)):
        _refused(call(**kw), "sst_blur", "null pointer")
    _refused(call(y=x), "sst_blur", "y == x", "out of place")
    for B in (0, -1, 65536):
        _refused(call(B=B), "sst_blur", f"batch {B} outside [1, 65535]")
    for K in (1, 2, 4, 23, -3):
        _refused(call(K=K), "sst_blur", f"the blur window K = {K} must be odd and in 3..21")
    for H, W in ((0, 40), (48, 0), (32769, 40)):
        _refused(call(H=H, W=W), "sst_blur", f"image {W}x{H} outside 1..32768")
    _refused(call(H=10, W=40), "sst_blur", "the half window 10 (K = 21) must be smaller than the image's shorter side (40x10)")
    for off in (4, 8, 16):
        _refused(call(deg=p32 + off), "sst_blur", "deg must be 32-byte aligned")
