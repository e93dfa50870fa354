"""CPU: the diagnostic and the variant mode of ubdvss_amd/csrc/build.sh (one unit table for all three kinds of library) produce complete
libraries, and the stamp facility (ubdvss_amd/csrc/stamps.h) leaves nothing in the product library."""
import ctypes
import glob
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "ubdvss_amd", "csrc", "build.sh")
PRODUCT = os.path.join(ROOT, "ubdvss_amd", "libubd_hip.so")
OLD_SETTERS = ["ubd_debug_set_stamps" + s for s in ("", "_wino", "_wino6", "_pp", "_d16s", "_s123", "_sepb")]


def _build(*args):
    r = subprocess.run(["bash", BUILD, *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.fixture(scope="module")
def diag_lib():
    _build("diag")                       # incremental: a second full compile of the library the first time
    return ctypes.CDLL(os.path.join(ROOT, "tools", "_ab", "libubd_hip_diag.so"))


def _assert_complete(lib):
    from ubdvss_amd import _lib
    missing = [name for name in _lib.SIGNATURES if not hasattr(lib, name)]
    assert not missing, f"not exported: {missing}"


def test_diagnostic_library_is_complete_and_has_the_one_setter(diag_lib):
    _assert_complete(diag_lib)
    assert [s for s in OLD_SETTERS[1:] if hasattr(diag_lib, s)] == []
    diag_lib.ubd_build_id.restype = ctypes.c_char_p
    diag_lib.ubd_last_error.restype = ctypes.c_char_p
    assert len(diag_lib.ubd_build_id()) == 16                                 # carries the fingerprint as the product does
    # ubd_debug_set_stamps is the five-argument setter (host table only: no GPU needed): clearing a family succeeds, an unknown name is an error
    setter = diag_lib.ubd_debug_set_stamps
    setter.restype, setter.argtypes = ctypes.c_int, [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int]
    for family in ("stem23", "stem123", "wino", "wino6", "sep123_16", "dilconv16s", "sepb16", "sep_bwd", "dil_wgrad16", "postprocess", "loss"):
        assert setter(family.encode(), None, 0, 0, 0) == 0, family
    assert setter(b"sepb", None, 0, -1, 1) != 0
    assert b"sepb" in diag_lib.ubd_last_error()


def test_product_library_has_no_stamp_symbol():
    from ubdvss_amd import _lib
    product = _lib.load()
    assert [s for s in OLD_SETTERS if hasattr(product, s)] == []
    assert b"ubd_debug_" not in open(PRODUCT, "rb").read()                    # no exported name (the dynamic string table) and no string of the facility


def test_variant_library_is_complete():
    _build("variant", "loss_no_stream_order", "loss", "-DLOSS1_NO_STREAM_ORDER")
    lib = ctypes.CDLL(os.path.join(ROOT, "tools", "_ab", "loss_no_stream_order.so"))
    _assert_complete(lib)
    assert [s for s in OLD_SETTERS if hasattr(lib, s)] == []


def test_one_unit_table():
    """No other script names a unit's flags; the wrappers of the recipe are gone or name no unit."""
    units = open(BUILD).read().split('UNITS="')[1].split('"')[0].split()
    assert len(units) == len(glob.glob(os.path.join(ROOT, "ubdvss_amd", "csrc", "*.hip")))
    for name in ("build_diag.sh", "build_variant.sh"):
        path = os.path.join(ROOT, "tools", name)
        if os.path.exists(path):
            text = open(path).read()
            assert "-ffp-contract" not in text and not [u for u in units if u in text.split()], name
    for path in glob.glob(os.path.join(ROOT, "tools", "*.sh")):
        assert "-ffp-contract" not in open(path).read(), path
    for path in glob.glob(os.path.join(ROOT, "ubdvss_amd", "csrc", "*.h*")):
        if not path.endswith("stamps.h"):
            text = open(path).read()
            assert "s_memtime" not in text and "s_memrealtime" not in text, path
