"""The trial's scalar reduction, LM decision and host mirror carried by the
gated Jacobian pass behind it (MMBA_PATH_TRIAL_RED_FOLD = 1: every workgroup
of k_jac_ne_u reduces the trial's rows and decides itself, one extra
workgroup publishes) against the standalone k_reduce_multi launch (= 0).  The
rows are reduced in k_reduce_multi's tree order and the decision repeats
lm_decide's operations, so x, the ||f|| trace, fvec and the solve's counters
are equal bit for bit.

Every scene has >= 256 camera-frames, pose-only camera blocks and forward
differences, or the fused pass (and with it the fold) is not taken.  The
scenes by workgroup width of k_jac_ne_u: two waves (about 39 observations per
camera-frame), four (257), eight (1,027).  Seven-parameter camera blocks
(PC = 7): ``make_config(1, frames=257)`` is the pose + focal shot without
solved bundles, the only seven-parameter plan synthetic makes at this frame
count; where it takes the fused pass its undamped step norm comes from the
block-diagonal solve's own slot, not from a row of the trial (the decision's
other source of SL_DNORM).  Every scene's run with the key at 1 must count
folded trials (mmba_kernel_stats.trial_red_folds), so no comparison passes
because the fold quietly stood down.  synthetic has no bundle-adjustment scene with seven-parameter
blocks, so PC = 7 with the factorisation flag converted by the trial's back
substitution is not covered.
"""
import numpy as np
import pytest

from mayamatchmovesolver_amd import abi, synthetic as S
from mayamatchmovesolver_amd.solver import Context, Solver, host_array

pytestmark = pytest.mark.gpu

LMDIF = abi.SOLVER_TYPE_CMINPACK_LMDIF
FOLD = abi.PATH_TRIAL_RED_FOLD
COUNTERS = ("reason_number", "iterations", "function_evals", "outer_iterations")


def _nw2():
    prob = S.make_config(3, frames=257, scale=0.05)
    return prob, S.config_options(prob, iterations=8)


def _nw4():
    prob = S.make_config(3, frames=257, scale=0.33)
    return prob, S.config_options(prob, iterations=6)


def _nw8():
    prob = S.make_config(3, frames=257, scale=1.32)
    return prob, S.config_options(prob, iterations=4)


def _pc7():
    prob = S.make_config(1, frames=257, scale=0.02)
    return prob, S.config_options(prob, iterations=6)


def _nw2_lmdif():
    prob = S.make_config(3, frames=257, scale=0.05)
    # lmdif's maxfev counts the n FD evaluations of a Jacobian too
    its = 3 * (prob.num_params + 1) + 4
    return prob, S.config_options(prob, solver_type=LMDIF, iterations=its)


def _nw2_rejects():
    # eight times the spec's initial perturbation: half the trials are rejected
    prob = S.make_config(3, frames=257, scale=0.05, init_noise=8.0)
    return prob, S.config_options(prob, iterations=12)


def _nw2_converges():
    prob = S.make_config(3, frames=257, scale=0.05, obs_noise=0.0)
    return prob, S.config_options(prob)


SCENES = {
    "nw2": _nw2,
    "nw4": _nw4,
    "nw8": _nw8,
    "pc7": _pc7,
    "nw2_lmdif": _nw2_lmdif,
    "nw2_rejects": _nw2_rejects,
    "nw2_converges": _nw2_converges,
}
_built = {}
_ref = {}


def _scene(name):
    if name not in _built:
        _built[name] = SCENES[name]()
    return _built[name]


def _solve(prob, opt, ctx, out=None):
    """The solve, with the plan's count of folded trials
    (mmba_kernel_stats.trial_red_folds, read without the timing switch: timing
    spans make the fold stand down) as ``folds``."""
    s = Solver(prob, opt, context=ctx)
    try:
        r = s.solve(out=out)
        r.folds = s.kernel_stats()["trial_red_folds"]
        return r
    finally:
        s.close()


def _reference(name, ctx, paths):
    """The scene's solve with the standalone launch pinned, computed once."""
    if name not in _ref:
        paths(FOLD, 0)
        prob, opt = _scene(name)
        _ref[name] = _solve(prob, opt, ctx)
    return _ref[name]


def _assert_same(r, ref, msg=""):
    np.testing.assert_array_equal(r.x, ref.x, err_msg=msg)
    np.testing.assert_array_equal(r.fnorm_trace, ref.fnorm_trace, err_msg=msg)
    np.testing.assert_array_equal(r.fvec, ref.fvec, err_msg=msg)
    for k in COUNTERS:
        assert r.result[k] == ref.result[k], (msg, k)


@pytest.mark.parametrize("name", list(SCENES))
def test_fold_bit_identical(name, gpu_ctx, paths):
    ref = _reference(name, gpu_ctx, paths)
    assert ref.result["outer_iterations"] > 1
    assert ref.folds == 0
    paths(FOLD, 1)
    prob, opt = _scene(name)
    r = _solve(prob, opt, gpu_ctx)
    # the fold was taken: every trial behind which a Jacobian was enqueued,
    # so at least one per Jacobian after the first
    assert r.folds >= ref.result["outer_iterations"] - 1 > 0, (name, r.folds)
    _assert_same(r, ref, name)


def test_rejected_trials_close_the_gate(gpu_ctx, paths):
    """A closed gate, a damped re-solve and a later open gate: the reference
    run rejects trials (more evaluations than one per outer iteration)."""
    for name in ("nw2", "nw2_rejects"):
        g = _reference(name, gpu_ctx, paths).result
        assert g["function_evals"] > g["outer_iterations"] + 1, name


def test_reason_codes(gpu_ctx, paths):
    assert _reference("nw2", gpu_ctx, paths).result["reason_number"] == 5  # maxfev
    assert _reference("nw2_converges", gpu_ctx, paths).result["reason_number"] in (1, 2)


def test_plan_reuse(gpu_ctx, paths):
    """Three solves through one plan, each equal to a fresh plan's: the
    mirror, the sequence word and the flag's state carry across solves."""
    ref = _reference("nw2_rejects", gpu_ctx, paths)
    paths(FOLD, 1)
    prob, opt = _scene("nw2_rejects")
    s = Solver(prob, opt, context=gpu_ctx)
    try:
        runs = [s.solve() for _ in range(3)]
        folds = s.kernel_stats()["trial_red_folds"]
    finally:
        s.close()
    assert folds >= 3 * (ref.result["outer_iterations"] - 1) > 0
    for k, r in enumerate(runs):
        _assert_same(r, ref, "solve %d" % k)


PINS = {
    "pre_schur": {abi.PATH_PRE_SCHUR: 1},
    "trial_records_off": {abi.PATH_TRIAL_RECORDS: 0},
    "backsub_thread": {abi.PATH_BACKSUB_GROUP: 0},
    "handback_kernel": {abi.PATH_HANDBACK_DMA: 0},
    "handback_kernel_pre0": {abi.PATH_HANDBACK_DMA: 0, abi.PATH_PRE_HANDBACK: 0},
    "handback_kernel_pre1": {abi.PATH_HANDBACK_DMA: 0, abi.PATH_PRE_HANDBACK: 1},
}


@pytest.mark.parametrize("pin", list(PINS))
def test_fold_with_other_pins(pin, gpu_ctx, paths):
    """The fold beside the other pinned paths (with the speculative kernel
    hand-back it stands down); page-locked output lists where the hand-back
    kernel needs them."""
    ref = _reference("nw2", gpu_ctx, paths)
    prob, opt = _scene("nw2")
    for k, v in PINS[pin].items():
        paths(k, v)
    paths(FOLD, 1)
    out = None
    if abi.PATH_HANDBACK_DMA in PINS[pin]:
        out = (host_array(prob.num_residuals), host_array(prob.num_residuals),
               host_array(prob.num_obs))
    r = _solve(prob, opt, gpu_ctx, out=out)
    if PINS[pin].get(abi.PATH_PRE_HANDBACK, 1) == 1 and out is not None:
        assert r.folds == 0  # the speculative hand-back rides on the decision's slots
    else:
        assert r.folds > 0
    _assert_same(r, ref, pin)
    if out is not None:
        np.testing.assert_array_equal(out[0], ref.fvec)


def test_fold_stands_down_on_two_shards(paths):
    """A sharded plan reduces in its own launch whatever the key says."""
    prob = S.make_config(3, frames=40, scale=0.004)
    opt = S.config_options(prob, iterations=6)
    ctx = Context.multi([0, 0])
    try:
        runs = []
        for key in (0, 1):
            paths(FOLD, key)
            runs.append(_solve(prob, opt, ctx))
    finally:
        ctx.close()
    assert runs[0].result["outer_iterations"] > 1
    assert runs[0].folds == runs[1].folds == 0
    _assert_same(runs[1], runs[0], "two shards")
