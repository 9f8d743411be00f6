"""The shim's plan cache across changed marker values
(integration/adjust_mmba_core.cpp, tests/shim_refresh/shim_refresh_test.cpp):
marker positions and weights are no longer part of ``FlatScene::plan_key`` --
a cached plan takes them through ``mmba_plan_set_marker_values`` -- while the
observation list still is.

CPU: the key of the nudged scene equals the original's, the key of a scene
with another obs_frame list does not.  The -m gpu leg solves a scene, nudges
one marker and one weight, solves again: one cached plan, and the bits of a
shim whose first solve already saw the nudged scene."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "shim_refresh")
BASE, NUDGED, SHORTER = 0, 1, 2


@pytest.fixture(scope="module")
def drv():
    subprocess.check_call(["make", "-s", "-C", DIR])
    L = C.CDLL(os.path.join(DIR, "libshimrefresh.so"))
    dp = C.POINTER(C.c_double)
    L.refresh_solve.argtypes = [C.c_int, C.c_int, dp, dp, C.c_char_p, C.c_int]
    for f in (L.refresh_num_params, L.refresh_num_errors, L.refresh_cached_plans):
        f.argtypes = [C.c_int]
    L.refresh_keys_equal.argtypes = [C.c_int, C.c_int]
    L.refresh_release.restype = None
    return L


def test_plan_key_ignores_marker_values_not_structure(drv):
    assert drv.refresh_keys_equal(BASE, BASE) == 1
    assert drv.refresh_keys_equal(BASE, NUDGED) == 1
    assert drv.refresh_num_errors(SHORTER) == drv.refresh_num_errors(BASE) - 2
    assert drv.refresh_keys_equal(BASE, SHORTER) == 0


def shim_solve(drv, which, variant):
    n, m = drv.refresh_num_params(variant), drv.refresh_num_errors(variant)
    x, f = np.zeros(n), np.zeros(m)
    msg = C.create_string_buffer(256)
    dp = C.POINTER(C.c_double)
    st = drv.refresh_solve(which, variant, x.ctypes.data_as(dp), f.ctypes.data_as(dp), msg, 256)
    assert st == 1, msg.value
    return x, f


@pytest.mark.gpu
def test_gpu_nudged_scene_reuses_the_cached_plan(drv):
    try:
        x0, f0 = shim_solve(drv, 0, BASE)
        assert drv.refresh_cached_plans(0) == 1
        x1, f1 = shim_solve(drv, 0, NUDGED)
        assert drv.refresh_cached_plans(0) == 1  # the same plan, refreshed
        xf, ff = shim_solve(drv, 1, NUDGED)      # a shim that never saw the first scene
        assert drv.refresh_cached_plans(1) == 1
        np.testing.assert_array_equal(x1, xf)
        np.testing.assert_array_equal(f1, ff)
        assert not np.array_equal(f1, f0) and not np.array_equal(x1, x0)
        shim_solve(drv, 0, SHORTER)              # another structure: a second plan
        assert drv.refresh_cached_plans(0) == 2
    finally:
        drv.refresh_release()
