"""The trial back substitution with a group of four lanes per bundle
(MMBA_PATH_BACKSUB_GROUP, k_backsub_trial_g) against the thread-per-bundle
kernel, each in its two-pass (k_obs_wtx) and one-pass (MMBA_PATH_BACKSUB_ONEPASS)
form: every sum keeps its order, so x, the ||f|| trace and fvec are equal bit
for bit.  The scenes are the smallest at which the lane logic can go wrong:
idle groups in a workgroup, a bundle count that is no multiple of 64, a partly
filled second chunk of observations, tens of observations per bundle, globals
(the Wg term, the T.other workgroups), a bundle seen twice in a camera-frame,
bundles with a parent (the record by the table walk), a bundle with two solved
parameters, lmdif's difference step, and a sharded plan's ownership mask.
"""
import numpy as np
import pytest

from mayamatchmovesolver_amd import abi, make_options, synthetic as S
from mayamatchmovesolver_amd.solver import Context, Solver

pytestmark = pytest.mark.gpu

LMDER, LMDIF = abi.SOLVER_TYPE_CMINPACK_LMDER, abi.SOLVER_TYPE_CMINPACK_LMDIF
MMSG, DAG = abi.SCENE_GRAPH_MODE_MM_SCENE_GRAPH, abi.SCENE_GRAPH_MODE_MAYA_DAG
# (GROUP, ONEPASS); the first is the reference
FORMS = ((0, 0), (1, 0), (1, 1), (0, 1))


def _c4_f8():
    prob = S.make_config(3, frames=8, scale=0.001)
    return prob, S.config_options(prob, iterations=8), {}


def _c4_f300():
    prob = S.make_config(3, frames=300, scale=0.06)
    return prob, S.config_options(prob, iterations=12), {}


def _c4_six_obs():
    prob = S.make_config(3, frames=64, scale=0.004, window=6, depth=(4, 10))
    return prob, S.config_options(prob, iterations=8), {}


def _c3_dense():
    prob = S.make_config(2, frames=4, scale=0.002)
    return prob, S.config_options(prob, iterations=8), {abi.PATH_DENSE: 1}


def _witness():
    return S.witness_scene(n_witness=1, n_focal=1), make_options(), {}


def _edge_dup():
    return S.edge_scene(duplicate_markers=3), make_options(scene_graph_mode=DAG, iterations=100), {}


def _edge_parented():
    prob = S.edge_scene(parented=True, solve_bundles=True)
    return prob, make_options(scene_graph_mode=DAG, iterations=100), {}


def _known_test1():
    return S.known_scene("test1"), S.known_options("test1", LMDER, DAG), {}


def _c4_f8_lmdif():
    prob = S.make_config(3, frames=8, scale=0.001)
    # lmdif's maxfev counts the n FD evaluations of a Jacobian too
    its = 4 * (prob.num_params + 1) + 6
    return prob, S.config_options(prob, solver_type=LMDIF, iterations=its), {}


SCENES = {
    "c4_f8": _c4_f8,
    "c4_f300": _c4_f300,
    "c4_six_obs": _c4_six_obs,
    "c3_dense": _c3_dense,
    "witness_g4": _witness,
    "edge_dup": _edge_dup,
    "edge_parented": _edge_parented,
    "known_test1": _known_test1,
    "c4_f8_lmdif": _c4_f8_lmdif,
}


def _solve_forms(prob, opt, ctx, paths, pins):
    runs = {}
    for group, one in FORMS:
        for k, v in pins.items():
            paths(k, v)
        paths(abi.PATH_BACKSUB_GROUP, group)
        paths(abi.PATH_BACKSUB_ONEPASS, one)
        s = Solver(prob, opt, context=ctx)
        try:
            runs[(group, one)] = s.solve()
        finally:
            s.close()
    return runs


def _assert_equal_forms(runs):
    ref = runs[FORMS[0]]
    assert ref.result["iterations"] > 2
    for k, r in runs.items():
        np.testing.assert_array_equal(r.x, ref.x, err_msg=str(k))
        np.testing.assert_array_equal(r.fnorm_trace, ref.fnorm_trace, err_msg=str(k))
        np.testing.assert_array_equal(r.fvec, ref.fvec, err_msg=str(k))


@pytest.mark.parametrize("name", list(SCENES))
def test_group_forms_bit_identical(name, gpu_ctx, paths):
    prob, opt, pins = SCENES[name]()
    _assert_equal_forms(_solve_forms(prob, opt, gpu_ctx, paths, pins))


def test_group_forms_bit_identical_two_shards(paths):
    """A 40-frame C4 scene on two shards: each parameter is counted in
    ||D p||^2 and ||D x||^2 by its owner (TrialFold::own), loaded by the lane
    that owns the parameter."""
    prob = S.make_config(3, frames=40, scale=0.004)
    opt = S.config_options(prob, iterations=6)
    ctx = Context.multi([0, 0])
    try:
        runs = _solve_forms(prob, opt, ctx, paths, {})
    finally:
        ctx.close()
    _assert_equal_forms(runs)
