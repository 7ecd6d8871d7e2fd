"""What the CPU tests of the criteria's C-ABI entries (tests/test_ssim_abi.py, test_freq_abi.py, test_bp_abi.py, test_st_maps.py,
test_st_general.py) share.  A plain helper module."""
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


# ---- the two structure-tensor maps entries (sst_st_maps, sst_st_general_maps: the same outputs, the second with a scratch buffer)
FAKE = 0x1000          # stands for a device pointer in calls that are refused on the host: never dereferenced


def st_maps_call(entry, x=FAKE, gt=FAKE, Sx=None, Sgt=None, Fx=None, Fgt=None, d=None, tile_sums=None, scratch=FAKE, shape=(2, 40, 40),
                 sigma=0.5, rho=2.0):
    """-> (rc, message) of one call of a maps entry; scratch goes to sst_st_general_maps only."""
    extra = (scratch,) if entry == "sst_st_general_maps" else ()
    rc = getattr(lib(), entry)(x, gt, Sx, Sgt, Fx, Fgt, d, tile_sums, *extra, *shape, sigma, rho, 1, None)
    return rc, lib().sst_last_error()


# (arguments, what the message holds): refused on the host by either entry
ST_MAPS_REFUSALS = [
    (dict(x=None, Sx=FAKE), b"null pointer"),
    (dict(gt=None, Sgt=FAKE), b"Sgt needs gt"),
    (dict(gt=None, Fgt=FAKE), b"Fgt needs gt"),
    (dict(gt=None, d=FAKE), b"d needs gt"),
    (dict(gt=None, tile_sums=FAKE), b"tile_sums cannot be computed without gt"),
    (dict(), b"no output requested"),
    (dict(gt=None), b"no output requested"),
]


def st_maps_refuses(entry, kwargs, message):
    rc, err = st_maps_call(entry, **kwargs)
    assert rc == -1 and message in err, (rc, err)
