"""What the CPU tests of the criteria's C-ABI entries (tests/test_ssim_abi.py, test_freq_abi.py, test_bp_abi.py) share.  A plain helper
module."""
import ctypes

from test_abi_symbols import header_decls


def lib():
    from srganst import _abi
    return _abi.lib()


def refused(rc, *needles):
    """The entry that returned rc refused, and its message holds every needle."""
    msg = lib().sst_last_error().decode()
    assert rc != 0 and msg, (rc, msg)
    for n in needles:
        assert n in msg, msg


def exported_and_declared(names):
    """Each name is exported by the library, declared in include/srganst.h and known to _abi with the header's argument count."""
    from srganst import _abi
    decls = header_decls()
    so = ctypes.CDLL(_abi.LIB_PATH)
    for name in names:
        assert name in decls and name in _abi.SIGNATURES, name
        assert hasattr(so, name), f"{name} not exported by libsrganst.so"
        assert len(_abi.SIGNATURES[name][1]) == decls[name], name
