"""The gated passes with their operands loaded ahead of their stores
(MMBA_PATH_LOADS_FIRST = 1) against the forms that load them where they are
used (= 0):

* k_jac_ne_u: diag[p], x[p] and ||f||^2 of the block's parameters loaded
  ahead of the loop and parked in LDS, g indexed from the staged parameter
  list -- no global load behind the observation loop -- and the wave sums
  formed by vector-unit lane moves whose lane 0 adds the same subtree sums
  as the xor butterfly (wave_sum_lane0);
* k_ne_bnd_jb: diag, x of the bundle's parameters and ||f|| loaded with the
  first index loads, the three parameters through epi_param_pre;
* k_schur_obs: the bundle columns' offset and the block widths from one packed
  per-observation plan word, Lb[b] issued with b.

Only where and when operands are loaded differs; every operation and its
order is the same, so x, the ||f|| trace, fvec, the two error lists and the
solve's counters are equal bit for bit.

Scenes as in test_gpu_trial_red_fold.py (>= 256 camera-frames, or the fused
pass is not taken): two-wave workgroups (about 39 observations per
camera-frame, one partial round), four (257 on average, 57 to 300: a second
round of a few lanes on some camera-frames, none on others), eight (1,027 on
average: three rounds); ``make_config(1, frames=257)`` has
seven-parameter blocks and no solved bundle, so neither k_ne_bnd_jb nor
k_schur_obs is launched there.  Every run on an unsharded fused plan must
count folded trials (mmba_kernel_stats.trial_red_folds): only k_jac_ne_u
folds them, so no comparison passes because another Jacobian pass ran.

synthetic makes no scene whose bundles hang under an animated transform at
>= 256 frames.  The instances of k_jac_ne_u for such plans (GEN) keep the
loads behind the loop whatever the key says (parked ahead of it their four-
and eight-wave forms spill scalars), so the key changes nothing of theirs but
the bundle pass and k_schur_obs, which do not depend on GEN; they are covered
by the existing suite only.
"""
import os
import re

import numpy as np
import pytest

from mayamatchmovesolver_amd import abi, synthetic as S

gpu = pytest.mark.gpu

LMDIF = abi.SOLVER_TYPE_CMINPACK_LMDIF
KEY = getattr(abi, "PATH_LOADS_FIRST", None)
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
    # eight times the spec's initial perturbation: half the trials are
    # rejected -- a closed gate with the early loads already in flight
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
    from mayamatchmovesolver_amd.solver import Solver
    s = Solver(prob, opt, context=ctx)
    try:
        r = s.solve(out=out)
        r.folds = s.kernel_stats()["trial_red_folds"]
        return r
    finally:
        s.close()


def _reference(name, ctx, paths):
    """The scene's solve with the key at 0, computed once."""
    if name not in _ref:
        paths(KEY, 0)
        prob, opt = _scene(name)
        _ref[name] = _solve(prob, opt, ctx)
    return _ref[name]


def _assert_same(r, ref, msg=""):
    np.testing.assert_array_equal(r.x, ref.x, err_msg=msg)
    np.testing.assert_array_equal(r.fnorm_trace, ref.fnorm_trace, err_msg=msg)
    np.testing.assert_array_equal(r.fvec, ref.fvec, err_msg=msg)
    # the lists handed back: errorList is fvec, then ud->errorList and
    # errorDistanceList
    np.testing.assert_array_equal(r.err_user, ref.err_user, err_msg=msg)
    np.testing.assert_array_equal(r.err_dist, ref.err_dist, err_msg=msg)
    for k in COUNTERS:
        assert r.result[k] == ref.result[k], (msg, k)


def test_key_agrees_with_header():
    """abi.py's path keys are include/mmba.h's, the new one among them."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "mmba.h")) as fh:
        keys = dict((m.group(1), int(m.group(2))) for m in
                    re.finditer(r"^#define MMBA_PATH_(\w+)\s+(\d+)", fh.read(), re.M))
    assert keys["LOADS_FIRST"] == 30
    assert keys["NUM"] == 31
    for name, value in keys.items():
        assert getattr(abi, "PATH_" + name) == value, name
    mine = dict((k[5:], v) for k, v in vars(abi).items() if k.startswith("PATH_"))
    assert mine == keys
    assert sorted(v for k, v in keys.items() if k != "NUM") == list(range(1, keys["NUM"]))


@gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_loads_first_bit_identical(name, gpu_ctx, paths):
    ref = _reference(name, gpu_ctx, paths)
    assert ref.result["outer_iterations"] > 1
    assert ref.folds > 0, name  # the fused pass ran
    paths(KEY, 1)
    prob, opt = _scene(name)
    out = (np.zeros(prob.num_residuals), np.zeros(prob.num_residuals), np.zeros(prob.num_obs))
    r = _solve(prob, opt, gpu_ctx, out=out)
    assert r.folds == ref.folds > 0, (name, r.folds)
    _assert_same(r, ref, name)
    np.testing.assert_array_equal(out[0], ref.fvec)
    np.testing.assert_array_equal(out[1], ref.err_user)
    np.testing.assert_array_equal(out[2], ref.err_dist)


@gpu
def test_default_is_the_new_form(gpu_ctx, paths):
    """Unpinned, the plan's own choice gives the same bits."""
    ref = _reference("nw4", gpu_ctx, paths)
    paths(KEY, -1)
    prob, opt = _scene("nw4")
    _assert_same(_solve(prob, opt, gpu_ctx), ref, "unpinned")


@gpu
def test_scenes_reach_what_they_claim(gpu_ctx, paths):
    """Rejected trials (a closed gate), both ends of lmder, and the rounds of
    observations per camera-frame the scenes are named for."""
    for name in ("nw2", "nw2_rejects"):
        g = _reference(name, gpu_ctx, paths).result
        assert g["function_evals"] > g["outer_iterations"] + 1, name
    assert _reference("nw2", gpu_ctx, paths).result["reason_number"] == 5  # maxfev
    assert _reference("nw2_converges", gpu_ctx, paths).result["reason_number"] in (1, 2)
    # the launcher's workgroup width (mean observations per camera-frame,
    # rounded up: > 256 four waves, > 1024 eight) and the longest segment's
    # rounds of 64 x waves observations
    for name, lo, hi, waves, rounds in (("nw2", 1, 256, 2, 1), ("nw4", 257, 1024, 4, 2),
                                        ("nw8", 1025, 1 << 30, 8, 3)):
        prob, _ = _scene(name)
        per = -(-prob.num_obs // 257)
        assert lo <= per <= hi, (name, per)
        longest = int(np.bincount(np.asarray(prob.obs_frame)).max())
        assert -(-longest // (64 * waves)) == rounds, (name, longest)


@gpu
def test_plan_reuse(gpu_ctx, paths):
    """Three solves through one plan with the key at 1, each equal to the
    reference: the packed plan words and the LDS copies carry no state."""
    from mayamatchmovesolver_amd.solver import Solver
    ref = _reference("nw2_rejects", gpu_ctx, paths)
    paths(KEY, 1)
    prob, opt = _scene("nw2_rejects")
    s = Solver(prob, opt, context=gpu_ctx)
    try:
        runs = [s.solve() for _ in range(3)]
    finally:
        s.close()
    for k, r in enumerate(runs):
        _assert_same(r, ref, "solve %d" % k)


PINS = {
    "fold_off": {abi.PATH_TRIAL_RED_FOLD: 0},
    "jb_recompute": {abi.PATH_JB_RECOMPUTE: 1},
    "backsub_thread": {abi.PATH_BACKSUB_GROUP: 0},
    "pre_schur": {abi.PATH_PRE_SCHUR: 1},
}


@gpu
@pytest.mark.parametrize("pin", list(PINS))
def test_loads_first_with_other_pins(pin, gpu_ctx, paths):
    """The key beside the other pinned paths (each bit-identical to the
    default on its own, by its own test): the fold off (||f||^2 from the slot,
    not the workgroup's row), the bundle pass's recompute branch, the
    thread-per-bundle back substitution, k_schur_obs behind the gated
    Jacobian.  Page-locked output lists."""
    from mayamatchmovesolver_amd.solver import host_array
    ref = _reference("nw4", gpu_ctx, paths)
    prob, opt = _scene("nw4")
    for k, v in PINS[pin].items():
        paths(k, v)
    paths(KEY, 1)
    out = (host_array(prob.num_residuals), host_array(prob.num_residuals),
           host_array(prob.num_obs))
    r = _solve(prob, opt, gpu_ctx, out=out)
    assert (r.folds == 0) == (pin == "fold_off")
    _assert_same(r, ref, pin)
    np.testing.assert_array_equal(out[1][:prob.num_residuals], ref.err_user)
    np.testing.assert_array_equal(out[2][:prob.num_obs], ref.err_dist)


@gpu
def test_two_shards_on_one_device(paths):
    """A two-shard plan (own_cf / own_bnd: a shard's passes store only its own
    camera-frames' and bundles' scalars)."""
    from mayamatchmovesolver_amd.solver import Context
    prob = S.make_config(3, frames=300, scale=0.04)
    opt = S.config_options(prob, iterations=5)
    ctx = Context.multi([0, 0])
    try:
        runs = []
        for key in (0, 1):
            paths(KEY, key)
            runs.append(_solve(prob, opt, ctx))
    finally:
        ctx.close()
    assert runs[0].result["outer_iterations"] > 1
    _assert_same(runs[1], runs[0], "two shards")
