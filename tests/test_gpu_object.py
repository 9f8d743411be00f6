"""Object tracking: an animated transform above its bundles, solved at any
frame count.

A rigid object is a transform keyed per frame with its bundles parented under
it; its six pose curves are solved.  The reference re-measures only an
animated parameter's own frame for its FD column (adjust_solveFunc.cpp
frameIndexEnable), so such a column reaches the rows of its frame whose bundle
hangs under the object.  Plan::build puts it into the block of the one
camera-frame that reads it (VF_OBJ, MMBA_PATH_OBJ_CF) where the global arrow
would exceed 48 parameters -- 8 frames of a 6-DoF object before -- and the
generic kernels read the parent's world matrix from object records built once
per evaluation (mmba_object.hip, MMBA_PATH_OBJ_REC) instead of walking the
transform chain per observation and column.

Every scene (synthetic.OBJECT_TEST_SCENES; the oracle's own stability on each
is in profiles/r13_object/object_envelope.txt, all below 1e-8) is held to the
CPU oracle at the bars the other parity tests use: residuals rtol 1e-12, the
FD Jacobian within 1e-7 of its largest entry with the same zero pattern, whole
solves through tests.test_gpu_parity.check_solve (1e-6 on x and on the
per-evaluation ||f|| trace, equal counts)."""
import numpy as np
import pytest

from mayamatchmovesolver_amd import abi, synthetic as S
from mayamatchmovesolver_amd._lib import MmbaError
from mayamatchmovesolver_amd.solver import Solver
from tests.test_gpu_parity import REL, check_solve
from tests.test_object_host import object_params

pytestmark = pytest.mark.gpu

DAG, MMSG = abi.SCENE_GRAPH_MODE_MAYA_DAG, abi.SCENE_GRAPH_MODE_MM_SCENE_GRAPH
LMDER, LMDIF = abi.SOLVER_TYPE_CMINPACK_LMDER, abi.SOLVER_TYPE_CMINPACK_LMDIF
CF, BND, GLOB = 0, 1, 2  # mmba_plan_param_layout's classes


def scene(name, **over):
    return S.object_scene(**{**S.OBJECT_TEST_SCENES[name], **over})


def check_f_and_J(prob, opt, oracle, s):
    """Residuals and the dense FD Jacobian at x0 and off it; returns the last J."""
    for x in (np.asarray(prob.x0), np.asarray(prob.x0) + 0.01):
        f, _, ed, _ = s.measure(x)
        f_ref, _, ed_ref, _ = oracle.measure(prob, opt, x)
        np.testing.assert_allclose(f, f_ref, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(ed, ed_ref, rtol=1e-12, atol=1e-12)
        J = s.jacobian(x)
        _, J_ref = oracle.jacobian(prob, opt, x)
        big = np.max(np.abs(J_ref))
        assert np.max(np.abs(J - J_ref)) <= 1e-7 * big
        assert np.array_equal(J != 0, J_ref != 0) or np.max(np.abs(J[J_ref == 0])) < 1e-9 * big
    return J


def check_all(prob, opt, oracle, gpu_ctx, layout=None, reproject=False):
    s = Solver(prob, opt, context=gpu_ctx)
    try:
        if layout is not None:
            layout(*s.param_layout())
        J = check_f_and_J(prob, opt, oracle, s)
        if reproject:
            for x in (None, np.asarray(prob.x0) + 0.001):
                pts, mkr = s.reproject(x)
                pr, mr = oracle.reproject_obs(prob, opt, x)
                np.testing.assert_allclose(pts, pr, rtol=1e-12, atol=1e-12)
                np.testing.assert_allclose(mkr, mr, rtol=1e-12, atol=1e-12)
    finally:
        s.close()
    check_solve(prob, opt, oracle, gpu_ctx)
    return J


def all_in_own_frame_block(prob):
    """Every parameter in class 0, in the block of its own frame (one camera
    seen on every frame: camera-frame index = frame)."""
    def check(cls, blk):
        assert np.all(cls == CF), cls
        assert np.array_equal(blk, prob.param_frame)
    return check


# 1. above the cap: 54 object parameters, refused before with "48 global"
@pytest.mark.parametrize("mode", [DAG, MMSG])
@pytest.mark.parametrize("solver_type", [LMDER, LMDIF])
def test_above_the_cap(mode, solver_type, oracle, gpu_ctx):
    prob = scene("above_cap")
    assert prob.num_params == 54 > 48
    check_all(prob, S.object_options(mode, solver_type), oracle, gpu_ctx,
              layout=all_in_own_frame_block(prob), reproject=True)


# 2. 10 frames: 10 record sets of 7 slots, 70 threads -- a second workgroup
# of k_obj_records (9 frames: 63, one workgroup)
def test_records_cross_a_workgroup(oracle, gpu_ctx):
    prob = scene("crosses_workgroup")
    check_all(prob, S.object_options(), oracle, gpu_ctx, layout=all_in_own_frame_block(prob))


# 3. solved bundles under the object (generic bundles: bnd_p4.w = -1)
def test_solved_bundles_under_the_object(oracle, gpu_ctx):
    prob = scene("solved_bundles")
    op = object_params(prob)

    def layout(cls, blk):
        assert np.all(cls[op] == CF) and np.array_equal(blk[op], prob.param_frame[op])
        rest = np.setdiff1d(np.arange(prob.num_params), op)
        assert np.all(cls[rest] == BND)
        assert sorted(set(blk[rest].tolist())) == [3, 4, 5]  # bundles 0..2 hold the gauge
    check_all(prob, S.object_options(), oracle, gpu_ctx, layout=layout)


@pytest.mark.parametrize("lam", [1.0, 1e-3])
def test_solved_bundles_damped_step(lam, gpu_ctx):
    """The damped step of one LM iteration against the dense solve of
    (J^T J + lam D^2) p = J^T f formed from the returned fjac, at the bars of
    tests/test_gpu_damped_step.py (its module docstring)."""
    from tests.test_gpu_damped_step import check_bars
    prob = scene("solved_bundles")
    s = Solver(prob, S.object_options(), context=gpu_ctx)
    try:
        step, g, diag, J = s.damped_step(prob.x0, lam)
        f = s.measure(prob.x0)[0]
    finally:
        s.close()
    check_bars("object_solved_bundles", lam, dict(out={lam: (step, g, diag)}, J=J, f=f, ref=None))


# 4. solved camera + object + scene bundles: blocks of 12 = PCMAX
def test_solved_camera_and_object(oracle, gpu_ctx):
    kw = S.OBJECT_TEST_SCENES["solved_camera"]
    prob = scene("solved_camera")
    op = object_params(prob)
    F, B = kw["frames"], kw["bundles"]

    def layout(cls, blk):
        anim = prob.param_frame >= 0
        assert np.all(cls[anim] == CF) and np.array_equal(blk[anim], prob.param_frame[anim])
        assert np.all(cls[~anim] == BND)
        assert np.bincount(blk[anim], minlength=F).tolist() == [6] + [12] * (F - 1)
    J = check_all(prob, S.object_options(), oracle, gpu_ctx, layout=layout)
    # a scene bundle's rows: camera columns, exact zeros in the object's
    rows = np.flatnonzero(np.asarray(prob.mkr_bnd)[prob.obs_marker] >= B)
    rows = np.concatenate([2 * rows, 2 * rows + 1])
    assert np.all(J[np.ix_(rows, op)] == 0.0)
    assert np.any(J[rows] != 0.0)


# 5. visibility windows, and an object-frame no row reads
def test_windows_and_a_blind_frame(oracle, gpu_ctx):
    kw = S.OBJECT_TEST_SCENES["windows"]
    prob = scene("windows")
    J = check_all(prob, S.object_options(), oracle, gpu_ctx, layout=all_in_own_frame_block(prob))
    blind = np.flatnonzero(prob.param_frame == kw["frames"] - 1)
    assert blind.size == 6 and np.all(J[:, blind] == 0.0)


# 6. the object under a rotated, scaled group; the group's rotation solved:
# record variants for bundle-side globals beside the block parameters
@pytest.mark.parametrize("name", ["parent", "parent_solved"])
def test_object_under_a_group(name, oracle, gpu_ctx):
    prob = scene(name)
    op = object_params(prob)

    def layout(cls, blk):
        assert np.all(cls[op] == CF) and np.array_equal(blk[op], prob.param_frame[op])
        rest = np.setdiff1d(np.arange(prob.num_params), op)
        assert rest.size == (3 if name == "parent_solved" else 0)
        assert np.all(cls[rest] == GLOB) and np.all(blk[rest] == -1)
    check_all(prob, S.object_options(), oracle, gpu_ctx, layout=layout)


# 7. records against the chain walk
@pytest.mark.parametrize("name", ["above_cap", "solved_bundles", "parent_solved"])
def test_records_and_chain_walk(name, oracle, gpu_ctx, paths):
    prob = scene(name)
    opt = S.object_options()
    x = np.asarray(prob.x0) + 0.01
    fs = {}
    for rec in (0, 1):
        paths(abi.PATH_OBJ_REC, rec)
        check_all(prob, opt, oracle, gpu_ctx)
        s = Solver(prob, opt, context=gpu_ctx)
        try:
            fs[rec] = s.measure(x)[0]
        finally:
            s.close()
    np.testing.assert_allclose(fs[1], fs[0], rtol=1e-13, atol=0.0)


# 8. below the cap: the globals as before unless pinned
@pytest.mark.parametrize("pin", [-1, 1])
def test_below_the_cap(pin, oracle, gpu_ctx, paths):
    prob = scene("below_cap")
    assert prob.num_params == 36 <= 48
    paths(abi.PATH_OBJ_CF, pin)

    def layout(cls, blk):
        if pin == 1:
            all_in_own_frame_block(prob)(cls, blk)
        else:
            assert np.all(cls == GLOB) and np.all(blk == -1)
    check_all(prob, S.object_options(), oracle, gpu_ctx, layout=layout)


# 9. what stays refused, and says why
def refused(prob, opt, gpu_ctx):
    with pytest.raises(MmbaError) as e:
        Solver(prob, opt, context=gpu_ctx).close()
    return str(e.value)


def test_refused_with_the_form_pinned_off(gpu_ctx, paths):
    paths(abi.PATH_OBJ_CF, 0)
    msg = refused(scene("above_cap"), S.object_options(), gpu_ctx)
    assert "48 global" in msg and "MMBA_PATH_OBJ_CF = 0" in msg


def test_refused_seen_by_two_cameras(gpu_ctx):
    msg = refused(scene("above_cap", cameras=2), S.object_options(), gpu_ctx)
    assert "48 global" in msg and "several cameras" in msg


def test_refused_central_differences(gpu_ctx):
    opt = S.object_options(auto_diff_type=abi.AUTO_DIFF_TYPE_CENTRAL)
    msg = refused(scene("above_cap"), opt, gpu_ctx)
    assert "48 global" in msg and "central differences" in msg


def test_refused_two_objects_and_a_solved_camera(gpu_ctx):
    msg = refused(scene("above_cap", objects=2, solve_camera=True), S.object_options(), gpu_ctx)
    assert "more than 12 parameters on one camera-frame" in msg


# 10. a cached plan: new attribute values, then a solve -- the records follow
def test_plan_cache_rebuilds_the_records(oracle, gpu_ctx):
    from tests.test_gpu_plan_cache import written_back
    prob = scene("above_cap")
    opt = S.object_options()
    s = Solver(prob, opt, context=gpu_ctx)
    try:
        first = s.solve()
        prob2 = written_back(prob, first.x + 0.01)
        xr, _f, _eu, _ed, rr, trr = oracle.solve(prob2, opt)
        s.set_attr_values(prob2.attr_values)
        out = s.solve(x0=prob2.x0)
    finally:
        s.close()
    g = out.result
    assert (g["reason_number"], g["iterations"], g["function_evals"], g["jacobian_evals"]) == \
        (rr.reason_number, rr.iterations, rr.function_evals, rr.jacobian_evals)
    np.testing.assert_allclose(out.fnorm_trace, trr, rtol=REL, atol=1e-9 * trr[0])
    assert np.max(np.abs(out.x - xr) / np.maximum(np.abs(xr), 1e-3)) <= REL
