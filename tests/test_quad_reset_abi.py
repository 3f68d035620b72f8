"""The quadruped's masked reset on the surfaces that need no GPU: include/allsteps.h declares as_quad_reset_mask,
the library exports it and _native's table names it, AnymalCStonesEnv has _reset_idx, and null arguments come back
as AS_ERR_INVALID before any device call."""

import ctypes as C
import inspect
import os
import re

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "allsteps.h")


def test_header_declares_the_masked_reset_beside_reset_all():
    src = open(HEADER).read()
    m = re.search(r"^int\s+as_quad_reset_mask\(([^)]*)\);", src, re.M)
    assert m, "as_quad_reset_mask is not declared in allsteps.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert args == ["as_env_t* env", "const uint8_t* mask", "float* obs", "void* stream"]
    assert src.index("int as_quad_reset_all(") < m.start() < src.index("as_generate_stones(")


def test_native_table_and_library_export_it():
    from allsteps_isaaclab_amd import _native

    assert "as_quad_reset_mask" in _native.EXPORTED_SYMBOLS
    L = _native.load()
    assert hasattr(L, "as_quad_reset_mask")
    assert len(L.as_quad_reset_mask.argtypes) == 4
    assert list(inspect.signature(_native.NativeEnv.quad_reset_mask).parameters) == ["self", "mask", "obs", "stream"]


def test_env_has_reset_idx():
    from allsteps_isaaclab_amd.envs.anymal_c_stones_env import AnymalCStonesEnv

    assert list(inspect.signature(AnymalCStonesEnv._reset_idx).parameters) == ["self", "env_ids"]
    assert "_reset_idx" in vars(AnymalCStonesEnv)  # its own, not inherited


def test_null_arguments_return_invalid():
    from allsteps_isaaclab_amd import _native

    L = _native.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    # (a non-null handle is never dereferenced here: the null checks come first)
    for args in ((None, p, p, None), (p, None, p, None), (p, p, None, None), (None, None, None, None)):
        assert L.as_quad_reset_mask(*args) == -1
        assert b"as_quad_reset_mask: null argument" in L.as_last_error()
