"""The round-7 kernel options (csrc/options.cpp): defaults, set and revert through the C ABI.  Host logic only."""
import ctypes as C
import os

import pytest

from mlic_amd import _lib

# name -> (environment variable, default, values a set keeps as they are)
OPTIONS = {"lrp_half": ("MLIC_LRP_HALF", 0, False), "intra_half": ("MLIC_INTRA_HALF", 0, True),
           "gdn_skip": ("MLIC_GDN_SKIP", 1, False)}


def _get(name):
    v = C.c_int(-99)
    _lib.call("mlic_get_kernel_option", name.encode(), C.byref(v))
    return v.value


@pytest.mark.parametrize("name", sorted(OPTIONS))
def test_option_default_set_and_revert(name):
    var, default, raw = OPTIONS[name]
    if var in os.environ:  # the variable stands in for the built-in default (atoi of a plain integer)
        e = int(os.environ[var])
        default = e if raw else int(e != 0)
    assert _get(name) == default
    try:
        for v in (0, 1, 2):
            _lib.call("mlic_set_kernel_option", name.encode(), v)
            assert _get(name) == (v if raw else int(v != 0))
    finally:
        _lib.call("mlic_set_kernel_option", name.encode(), -1)
    assert _get(name) == default
