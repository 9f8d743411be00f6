"""Per-frame object tracking in one launch: the camera locked, the object's
bundles surveyed, its six pose curves solved frame by frame
(FrameSolveMode::kPerFrame) -- every frame's solve in one k_batch_lm launch
(its object form, mmba_batch_obj.hip) on a plan of
mmba_plan_create_per_frame, held to the CPU oracle run frame by frame.

The cases and their oracle results are those of
tests/test_perframe_object_host.py (which holds the oracle itself to them);
the bars are tests.test_gpu_perframe.check_frames' own: per frame the reason
and every counter equal, every error statistic and x within 1e-6 relative.
``Solver.batch_launches()`` tells the one-launch path from the
one-plan-per-frame fallback."""
import numpy as np
import pytest

from mayamatchmovesolver_amd import abi, synthetic as S
from mayamatchmovesolver_amd._lib import MmbaError
from mayamatchmovesolver_amd.solver import Solver, solve_per_frame
from tests.test_gpu_perframe import check_frames, oracle_per_frame
from tests.test_perframe_object_host import CASES, case

pytestmark = pytest.mark.gpu

CF = 0  # mmba_plan_param_layout's camera-frame class


def run_plan(name, oracle, gpu_ctx, interrupt=None, calls=1):
    """The case on a per-frame plan: layout, `calls` one-launch solves, each
    against the oracle."""
    prob, opt, xr, rr = case(name, oracle)
    s = Solver(prob, opt, context=gpu_ctx, per_frame=True)
    try:
        cls, blk = s.param_layout()
        assert np.all(cls == CF), cls
        assert np.array_equal(blk, prob.param_frame)  # one camera: block = frame
        for _ in range(calls):
            n0 = s.batch_launches()
            x, res = s.solve_per_frame(interrupt=interrupt)
            assert s.batch_launches() == n0 + 1
            check_frames(prob, res, rr, x, xr)
    finally:
        s.close()
    return res


# 1. the per-frame plan against the oracle
PLAN_CASES = sorted(n for n in CASES
                    if not n.startswith(("bounded", "opt-", "interrupt")))


@pytest.mark.parametrize("name", PLAN_CASES)
def test_per_frame_plan_matches_oracle(name, oracle, gpu_ctx):
    res = run_plan(name, oracle, gpu_ctx)
    if name == "windows":  # the blind frame: six exact-zero columns
        assert res[-1]["function_evals"] == 1 and res[-1]["error_is_better"] == 1


# 2. bounds: flipped difference signs, frames that are not written back
@pytest.mark.parametrize("name", ["bounded_small", "bounded_above_cap"])
def test_bounded_twins(name, oracle, gpu_ctx):
    res = run_plan(name, oracle, gpu_ctx)
    better = [g["error_is_better"] for g in res]
    assert 0 in better and 1 in better


# 3. options
@pytest.mark.parametrize("name", sorted(n for n in CASES if n.startswith("opt-")))
def test_options(name, oracle, gpu_ctx):
    run_plan(name, oracle, gpu_ctx)


def test_interrupt_pending(oracle, gpu_ctx):
    res = run_plan("interrupt_pending", oracle, gpu_ctx, interrupt=lambda: True)
    assert all(g["reason_number"] == -1 for g in res)


# 4. the one-shot entry: one launch, and the per-frame plans it falls back to
@pytest.mark.parametrize("name", ["small-dag-lmder", "above_cap-dag-lmder"])
def test_one_shot_takes_one_launch(name, oracle, gpu_ctx):
    prob, opt, xr, rr = case(name, oracle)
    n0 = Solver.batch_launches()
    x, res = solve_per_frame(prob, opt, context=gpu_ctx)
    assert Solver.batch_launches() == n0 + 1
    check_frames(prob, res, rr, x, xr)


@pytest.mark.parametrize("name", ["small-dag-lmder", "above_cap-dag-lmder"])
def test_one_shot_per_frame_plans(name, oracle, gpu_ctx, paths):
    prob, opt, xr, rr = case(name, oracle)
    paths(abi.PATH_PERFRAME_BATCH, 0)
    n0 = Solver.batch_launches()
    x, res = solve_per_frame(prob, opt, context=gpu_ctx)
    assert Solver.batch_launches() == n0
    check_frames(prob, res, rr, x, xr)


# 5. default plans: the block form above the 48-global cap, globals below it
def test_default_plan_above_the_cap(oracle, gpu_ctx):
    prob, opt, xr, rr = case("above_cap-dag-lmder", oracle)
    s = Solver(prob, opt, context=gpu_ctx)
    try:
        x, res = s.solve_per_frame()
    finally:
        s.close()
    check_frames(prob, res, rr, x, xr)


def test_default_plan_below_the_cap_names_the_constructor(oracle, gpu_ctx):
    prob, opt, _xr, _rr = case("small-dag-lmder", oracle)
    s = Solver(prob, opt, context=gpu_ctx)
    try:
        with pytest.raises(MmbaError) as e:
            s.solve_per_frame()
    finally:
        s.close()
    assert e.value.code == abi.MMBA_ERR_UNSUPPORTED
    assert "mmba_plan_create_per_frame" in str(e.value)


# 6. reuse: equal results call after call, then new attribute values
def test_plan_reuse_and_new_attribute_values(oracle, gpu_ctx):
    from tests.test_gpu_plan_cache import written_back
    prob, opt, xr, rr = case("above_cap-dag-lmder", oracle)
    s = Solver(prob, opt, context=gpu_ctx, per_frame=True)
    try:
        x1, res1 = s.solve_per_frame()
        x2, res2 = s.solve_per_frame()
        _same(res1, res2, x1, x2)
        check_frames(prob, res1, rr, x1, xr)
        prob2 = written_back(prob, x1 + 0.01)
        xr2, rr2 = oracle_per_frame(prob2, opt, oracle)
        s.set_attr_values(prob2.attr_values)
        x3, res3 = s.solve_per_frame(x0=prob2.x0)
    finally:
        s.close()
    check_frames(prob2, res3, rr2, x3, xr2)


def _same(res1, res2, x1, x2):
    """Equal but for the wall-clock fields."""
    for a, b in zip(res1, res2):
        assert {k: v for k, v in a.items() if not k.startswith("time_")} == \
            {k: v for k, v in b.items() if not k.startswith("time_")}
    assert np.array_equal(x1, x2)


# 7. what stays refused, and says why
def refused(prob, opt, gpu_ctx):
    s = Solver(prob, opt, context=gpu_ctx, per_frame=True)
    try:
        with pytest.raises(MmbaError) as e:
            s.solve_per_frame()
    finally:
        s.close()
    assert e.value.code == abi.MMBA_ERR_UNSUPPORTED
    return str(e.value)


def test_refused_seen_by_two_cameras(gpu_ctx):
    msg = refused(S.object_scene(frames=3, bundles=6, cameras=2), S.object_options(), gpu_ctx)
    assert "several cameras" in msg


def test_refused_static_parameters(gpu_ctx):
    msg = refused(S.object_scene(frames=3, bundles=6, solve_bundles=True), S.object_options(),
                  gpu_ctx)
    assert "static" in msg


def test_refused_with_the_form_pinned_off(gpu_ctx, paths):
    paths(abi.PATH_OBJ_CF, 0)
    msg = refused(S.object_scene(frames=3, bundles=6), S.object_options(), gpu_ctx)
    assert "MMBA_PATH_OBJ_CF = 0" in msg


def test_whole_shot_entries_refuse_a_per_frame_plan(oracle, gpu_ctx):
    prob, opt, _xr, _rr = case("small-dag-lmder", oracle)
    s = Solver(prob, opt, context=gpu_ctx, per_frame=True)
    try:
        for call in (s.solve, s.measure):
            with pytest.raises(MmbaError) as e:
                call()
            assert e.value.code == abi.MMBA_ERR_INVALID
            assert "per-frame plan" in str(e.value)
    finally:
        s.close()
