"""``mmba_plan_set_marker_values`` without a device: the symbol is part of the
additive ABI 12 surface, and ``Solver.set_marker_values`` checks the arrays'
sizes against the plan's problem before anything reaches the library."""
import subprocess

import numpy as np
import pytest

from mayamatchmovesolver_amd import _lib, abi, synthetic as S
from mayamatchmovesolver_amd.solver import Solver


def test_symbol_exported_and_abi_stays_12():
    assert abi.ABI_VERSION == 12
    assert "mmba_plan_set_marker_values" in abi.EXPORTED_SYMBOLS
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert "mmba_plan_set_marker_values" in exported
    L = _lib.lib()
    assert L.mmba_abi_version() == 12
    assert len(L.mmba_plan_set_marker_values.argtypes) == 4


class _NoLibrary:
    """Stands where the library handle would: any use fails the test."""

    def __getattr__(self, name):
        raise AssertionError("the library was called (%s)" % name)


@pytest.fixture
def planless(monkeypatch):
    """A Solver over a problem with no plan behind it, and a library that
    refuses every call."""
    from mayamatchmovesolver_amd import solver
    monkeypatch.setattr(solver, "lib", lambda: _NoLibrary())
    s = object.__new__(Solver)
    s.problem = S.b4_scene(frames=4, bundles=6, frame_xy=True)
    s._h = None
    return s


@pytest.mark.parametrize("which,delta", [("obs_xy", -2), ("obs_xy", 2), ("obs_weight", 1),
                                         ("obs_weight", -1), ("mkr_frame_xy", 2)])
def test_wrong_sizes_are_rejected_before_any_c_call(planless, which, delta):
    p = planless.problem
    good = dict(obs_xy=p.obs_xy, obs_weight=p.obs_weight, mkr_frame_xy=p.mkr_frame_xy)
    n = good[which].size + delta
    bad = dict(good, **{which: np.resize(good[which], n)})
    before = {k: v.copy() for k, v in good.items()}
    with pytest.raises(ValueError, match=which):
        planless.set_marker_values(**bad)
    with pytest.raises(ValueError, match=which):  # alone, the others left as they are
        planless.set_marker_values(**{which: bad[which]})
    for k, v in before.items():  # the Problem is not touched
        np.testing.assert_array_equal(getattr(p, k), v)


def test_right_sizes_reach_the_library(planless):
    p = planless.problem
    with pytest.raises(AssertionError, match="mmba_plan_set_marker_values"):
        planless.set_marker_values(p.obs_xy, p.obs_weight, p.mkr_frame_xy)
