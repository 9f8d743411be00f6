"""A Jacobian enqueued ahead of the host's decision (Plan::pre_jac_enqueue)
against the same Jacobian launched by jac() itself: both take their fused
epilogue from one builder, so a solve that runs ahead and one that does not
are equal bit for bit in x, the ||f|| trace, fvec and the solve's counters.

The second run passes an interrupt callback that never asks to stop.  With a
callback set pre_jac_ok() is false, so every Jacobian is launched by jac()
after the host has read the trial; nothing else differs.  Each pair asserts
mmba_kernel_stats.trial_red_folds: greater than 0 without the callback (a
Jacobian ran ahead and carried the trial's reduction), 0 with it.

The scenes are the smallest that take the fused pass (>= 256 camera-frames,
as in test_gpu_trial_red_fold.py): accepted trials only, rejected trials with
closed gates, and the seven-parameter plan without a solved bundle whose
undamped step is the block-diagonal one-launch solve.
"""
import numpy as np
import pytest

from mayamatchmovesolver_amd import synthetic as S
from mayamatchmovesolver_amd.solver import Solver

pytestmark = pytest.mark.gpu

COUNTERS = ("reason_number", "iterations", "function_evals", "outer_iterations")


def _accepts():
    prob = S.make_config(3, frames=257, scale=0.05)
    return prob, S.config_options(prob, iterations=8)


def _rejects():
    prob = S.make_config(3, frames=257, scale=0.05, init_noise=8.0)
    return prob, S.config_options(prob, iterations=12)


def _pc7():
    prob = S.make_config(1, frames=257, scale=0.02)
    return prob, S.config_options(prob, iterations=6)


SCENES = {"accepts": _accepts, "rejects": _rejects, "pc7": _pc7}


def _solve(prob, opt, ctx, interrupt=None):
    s = Solver(prob, opt, context=ctx)
    try:
        r = s.solve(interrupt=interrupt)
        r.folds = s.kernel_stats()["trial_red_folds"]
        return r
    finally:
        s.close()


@pytest.mark.parametrize("name", list(SCENES))
def test_ahead_equals_jac(name, gpu_ctx):
    prob, opt = SCENES[name]()
    ahead = _solve(prob, opt, gpu_ctx)
    assert ahead.result["outer_iterations"] > 1
    assert ahead.folds > 0, name  # a Jacobian ran ahead of the host's decision
    own = _solve(prob, opt, gpu_ctx, interrupt=lambda: False)
    assert own.folds == 0, name   # every Jacobian launched by jac() itself
    np.testing.assert_array_equal(own.x, ahead.x, err_msg=name)
    np.testing.assert_array_equal(own.fnorm_trace, ahead.fnorm_trace, err_msg=name)
    np.testing.assert_array_equal(own.fvec, ahead.fvec, err_msg=name)
    for k in COUNTERS:
        assert own.result[k] == ahead.result[k], (name, k)
