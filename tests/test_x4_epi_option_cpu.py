"""The "x4_epi" kernel option (csrc/options.cpp; conv_x4's lean epilogue: 0 off, 1 the default tile classes, 2 every
class): default, set and revert through the C ABI.  Host logic only."""
import ctypes as C
import os

from mlic_amd import _lib


def _get(name):
    v = C.c_int(-99)
    _lib.call("mlic_get_kernel_option", name.encode(), C.byref(v))
    return v.value


def test_x4_epi_default_set_and_revert():
    default = 1
    if "MLIC_X4_EPI" in os.environ:  # the variable stands in for the built-in default (atoi of a plain integer)
        default = int(os.environ["MLIC_X4_EPI"])
    assert _get("x4_epi") == default
    try:
        for v in (0, 1, 2):
            _lib.call("mlic_set_kernel_option", b"x4_epi", v)
            assert _get("x4_epi") == v
    finally:
        _lib.call("mlic_set_kernel_option", b"x4_epi", -1)
    assert _get("x4_epi") == default
