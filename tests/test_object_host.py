"""Object tracking scenes (synthetic.object_scene), CPU side: the parameter
structure the plan's object-frame classification rests on, and the oracle's
own solves of every scene tests/test_gpu_object.py holds the device to --
each ends by one of MINPACK's convergence tests (reason 1..3) with the final
||f|| below 0.2 of the first.  The oracle's stability on them (its x under a
1-ulp change of x0) is recorded by tools/object_envelope.py."""
import numpy as np
import pytest

from mayamatchmovesolver_amd import abi, synthetic as S

DAG, MMSG = abi.SCENE_GRAPH_MODE_MAYA_DAG, abi.SCENE_GRAPH_MODE_MM_SCENE_GRAPH
LMDER, LMDIF = abi.SOLVER_TYPE_CMINPACK_LMDER, abi.SOLVER_TYPE_CMINPACK_LMDIF


def object_params(prob, o=0):
    """Indices of the parameters on object o's six pose attributes."""
    return np.flatnonzero(np.isin(prob.param_attr, prob.meta["object_attrs"][o]))


@pytest.mark.parametrize("name", sorted(S.OBJECT_TEST_SCENES))
def test_parameter_structure(name):
    kw = S.OBJECT_TEST_SCENES[name]
    prob = S.object_scene(**kw)
    F, B = kw["frames"], kw["bundles"]
    op = object_params(prob)
    assert op.size == 6 * F
    assert np.all(prob.param_frame[op] >= 0)
    assert np.array_equal(np.bincount(prob.param_frame[op], minlength=F), np.full(F, 6))
    n = 6 * F
    if kw.get("solve_bundles"):
        n += 3 * (B - 3)  # the first three bundles hold the gauge
    if kw.get("solve_camera"):
        n += 6 * (F - 1) + 3 * 7  # frame 0 and scene bundle 0 locked
    if kw.get("parent") == "solve":
        n += 3
    assert prob.num_params == n
    static = np.setdiff1d(np.arange(n), op)
    if not kw.get("solve_camera"):
        assert np.all(prob.param_frame[static] < 0)
    # every object bundle hangs under the object's transform, which hangs
    # under the group when there is one
    otfm = int(np.flatnonzero(np.all(np.asarray(prob.tfm_attrs).reshape(-1, 9)[:, :6] ==
                                     np.asarray(prob.meta["object_attrs"][0]), axis=1))[0])
    par = np.asarray(prob.tfm_parent)
    assert np.all(par[np.asarray(prob.bnd_tfm)[:B]] == otfm)
    assert (par[otfm] >= 0) == bool(kw.get("parent"))


def test_windows_leave_a_blind_object_frame():
    kw = S.OBJECT_TEST_SCENES["windows"]
    prob = S.object_scene(**kw)
    F, B = kw["frames"], kw["bundles"]
    obj = np.asarray(prob.mkr_bnd)[prob.obs_marker] < B
    per_frame = np.bincount(prob.obs_frame[obj], minlength=F)
    assert per_frame[F - 1] == 0 and np.all(per_frame[:F - 1] >= 3)
    assert per_frame.min() < per_frame.max()
    # ... while the camera-frame itself has rows (the scene bundles)
    assert np.bincount(prob.obs_frame[~obj], minlength=F)[F - 1] == 8


CASES = [(name, DAG, LMDER) for name in sorted(S.OBJECT_TEST_SCENES)] + \
        [("above_cap", MMSG, LMDER), ("above_cap", DAG, LMDIF), ("above_cap", MMSG, LMDIF)]


@pytest.mark.parametrize("name,mode,solver_type", CASES)
def test_oracle_converges(name, mode, solver_type, oracle):
    prob = S.object_scene(**S.OBJECT_TEST_SCENES[name])
    _x, f, _eu, _ed, res, trace = oracle.solve(prob, S.object_options(mode, solver_type))
    assert res.reason_number in (1, 2, 3), res.as_dict()
    assert np.linalg.norm(f) < 0.2 * trace[0], (trace[0], np.linalg.norm(f))
