"""``mmba_plan_set_marker_values`` (``Solver.set_marker_values``): new marker
positions and weights on a built plan give what a plan freshly built from
them gives, bit for bit -- the solve, its outputs, the deviation metrics and
the other entry points -- on every kind of plan, after a solve has left its
state behind.  The refreshed plan holds the host's ``std::sqrt`` of the
weights and the build's own expression of the rolling-shutter scanline time,
so the bar is equality, not a tolerance.  Refusals leave the plan untouched."""
import dataclasses

import numpy as np
import pytest

from mayamatchmovesolver_amd import abi, make_options, synthetic as S
from mayamatchmovesolver_amd._lib import MmbaError
from mayamatchmovesolver_amd.solver import Context, Solver

pytestmark = pytest.mark.gpu

DAG = abi.SCENE_GRAPH_MODE_MAYA_DAG


def perturbed(prob, seed, xy=True, weight=True):
    """A copy of the problem with obs_xy += 1e-3 N(0, 1) and obs_weight *=
    U(0.5, 2); mkr_frame_xy, where present, moves with obs_xy at the entries
    both hold and by noise of its own elsewhere."""
    rng = np.random.Generator(np.random.PCG64(seed))
    M = prob.num_obs
    d = 1e-3 * rng.standard_normal((M, 2))
    scale = rng.uniform(0.5, 2.0, M)
    kw = {}
    if xy:
        kw["obs_xy"] = (prob.obs_xy.reshape(M, 2) + d).reshape(-1)
        if prob.mkr_frame_xy is not None:
            K, F = prob.num_markers, int(prob.num_frames)
            fd = 1e-3 * rng.standard_normal((K, F, 2))
            fd[prob.obs_marker, prob.obs_frame] = d
            kw["mkr_frame_xy"] = (prob.mkr_frame_xy.reshape(K, F, 2) + fd).reshape(-1)
    if weight:
        kw["obs_weight"] = prob.obs_weight * scale
    return dataclasses.replace(prob, **kw)


def refresh(s, p2):
    s.set_marker_values(p2.obs_xy, p2.obs_weight, p2.mkr_frame_xy)


RESULT_KEYS = ("iterations", "function_evals", "error_initial_avg", "reason_number")


def assert_same_solve(a, b):
    for name in ("x", "fnorm_trace", "fvec", "err_user", "err_dist"):
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name), err_msg=name)
    for k in RESULT_KEYS:
        assert a.result[k] == b.result[k], k
    assert a.metrics.keys() == b.metrics.keys()
    for k in a.metrics:
        np.testing.assert_array_equal(a.metrics[k], b.metrics[k], err_msg=k)


def fused_scene():
    from tests.test_bounds_host import scene
    prob = scene("c4_f257")
    return prob, S.config_options(prob, iterations=4)


def cfg(index, iterations, **kw):
    def make():
        prob = S.make_config(index, **kw)
        return prob, S.config_options(prob, iterations=iterations)
    return make


def b4(frame_xy):
    def make():
        prob = S.b4_scene(frames=4, bundles=6, frame_xy=frame_xy)
        return prob, S.config_options(prob)
    return make


SCENES = {
    "block_diagonal": cfg(1, 8, frames=6, scale=0.05),
    "bundles_band": cfg(3, 8, frames=12, scale=0.05),
    "fused_257": fused_scene,
    "rolling_shutter": cfg(4, 6, frames=6, scale=0.05, rolling_shutter=0.5),
    "b4_frame_xy": b4(True),
    "b4_obs_xy": b4(False),
    "dag_rows": lambda: (S.edge_scene(stiffness=True), make_options(scene_graph_mode=DAG,
                                                                    iterations=40)),
    "object": lambda: (S.object_scene(frames=9, bundles=6), S.object_options()),
}
GROUP_SCENE = cfg(3, 2, frames=40, scale=0.004)


def fresh_solve(prob, opt, ctx):
    s = Solver(prob, opt, context=ctx)
    try:
        return s.solve(metrics=True)
    finally:
        s.close()


@pytest.mark.parametrize("name", list(SCENES))
def test_refresh_equals_fresh_plan(name, gpu_ctx):
    prob, opt = SCENES[name]()
    p2 = perturbed(prob, 5)
    s = Solver(prob, opt, context=gpu_ctx)
    try:
        first = s.solve(metrics=True)  # leaves its state behind
        refresh(s, p2)
        second = s.solve(metrics=True)
    finally:
        s.close()
    assert_same_solve(second, fresh_solve(p2, opt, gpu_ctx))
    assert not np.array_equal(first.fvec, second.fvec)  # the new values reached the device
    assert not np.array_equal(first.x, second.x)


def test_rolling_shutter_scene_changes_tau():
    """The rolling-shutter case moves obs_tau = rs (0.5 - y): its y
    perturbation changes the bits of every scanline time."""
    prob, _ = SCENES["rolling_shutter"]()
    assert np.any(prob.cam_rs_value != 0.0)
    y0, y1 = prob.obs_xy[1::2], perturbed(prob, 5).obs_xy[1::2]
    assert np.all(0.5 * (0.5 - y0) != 0.5 * (0.5 - y1))


def test_refresh_group_plan():
    """Two shards on one device through the multi-device context: every shard
    is refreshed, its own and its halo observations."""
    prob, opt = GROUP_SCENE()
    p2 = perturbed(prob, 6)

    def run(p, then=None):
        ctx = Context.multi([0, 0])
        try:
            s = Solver(p, opt, context=ctx)
            try:
                assert s.num_shards == 2
                out = [s.solve(metrics=True)]
                if then is not None:
                    refresh(s, then)
                    out.append(s.solve(metrics=True))
                return out
            finally:
                s.close()
        finally:
            ctx.close()

    first, second = run(prob, p2)
    assert_same_solve(second, run(p2)[0])
    assert not np.array_equal(first.fvec, second.fvec)


def test_refresh_comm_sharded_plan():
    """Communicator-sharded plans: every rank passes the whole arrays, no
    collective runs in the refresh."""
    from tests.test_gpu_sharded import run_sharded
    prob, opt = GROUP_SCENE()
    p2 = perturbed(prob, 6)

    def both(s):
        a = s.solve(metrics=True)
        refresh(s, p2)
        return a, s.solve(metrics=True)

    outs = run_sharded(prob, opt, 2, call=both)
    fresh = run_sharded(p2, opt, 2, call=lambda s: s.solve(metrics=True))
    for r in range(2):
        assert_same_solve(outs[r][1], fresh[r])
        assert not np.array_equal(outs[r][0].fvec, outs[r][1].fvec)


def test_refresh_per_frame_plan(gpu_ctx):
    prob = S.object_scene(frames=3, bundles=6)
    opt = S.object_options()
    p2 = perturbed(prob, 7)

    def frames(res):
        return [{k: v for k, v in r.items() if not k.startswith("time_")} for r in res]

    s = Solver(prob, opt, context=gpu_ctx, per_frame=True)
    try:
        x1, res1 = s.solve_per_frame()
        refresh(s, p2)
        x2, res2 = s.solve_per_frame()
    finally:
        s.close()
    f = Solver(p2, opt, context=gpu_ctx, per_frame=True)
    try:
        xf, resf = f.solve_per_frame()
    finally:
        f.close()
    np.testing.assert_array_equal(x2, xf)
    assert frames(res2) == frames(resf)
    assert not np.array_equal(x1, x2)


@pytest.mark.parametrize("name", ["block_diagonal", "b4_frame_xy"])
def test_other_entry_points_after_refresh(name, gpu_ctx):
    """measure, jacobian and reproject (its marker output reads obs_xy) on a
    refreshed plan against a fresh one."""
    prob, opt = SCENES[name]()
    p2 = perturbed(prob, 8)
    x = np.asarray(prob.x0) + 1e-3

    def calls(s):
        return (s.measure(x), s.measure(None), (s.jacobian(x),), s.reproject(x),
                s.reproject(None))

    s = Solver(prob, opt, context=gpu_ctx)
    try:
        s.solve()
        before = calls(s)
        refresh(s, p2)
        got = calls(s)
    finally:
        s.close()
    f = Solver(p2, opt, context=gpu_ctx)
    try:
        want = calls(f)
    finally:
        f.close()
    for g, w, b in zip(got, want, before):
        for ga, wa in zip(g, w):
            np.testing.assert_array_equal(ga, wa)
    assert not np.array_equal(got[0][0], before[0][0])
    assert not np.array_equal(got[3][1], before[3][1])  # reproject's markers


def test_stale_outputs_are_gone_after_refresh(gpu_ctx):
    """What a solve left for mmba_plan_outputs / mmba_plan_error_metrics does
    not describe the new measurements: both refuse as on a fresh plan until a
    solve or measure has run again."""
    prob, opt = SCENES["block_diagonal"]()
    p2 = perturbed(prob, 9)
    fresh = Solver(prob, opt, context=gpu_ctx)
    s = Solver(prob, opt, context=gpu_ctx)
    try:
        s.solve()
        s.outputs()
        s.error_metrics()
        refresh(s, p2)
        for plan in (fresh, s):
            for call in (plan.outputs, plan.error_metrics):
                with pytest.raises(MmbaError) as e:
                    call()
                assert e.value.code == abi.MMBA_ERR_INVALID
        s.measure(prob.x0)
        s.outputs()
        s.error_metrics()
    finally:
        s.close()
        fresh.close()


@pytest.mark.parametrize("part", ["weight", "xy"])
def test_partial_refresh(part, gpu_ctx):
    prob, opt = SCENES["bundles_band"]()
    p2 = perturbed(prob, 10, xy=part == "xy", weight=part == "weight")
    if part == "weight":
        np.testing.assert_array_equal(p2.obs_xy, prob.obs_xy)
    else:
        np.testing.assert_array_equal(p2.obs_weight, prob.obs_weight)
    s = Solver(prob, opt, context=gpu_ctx)
    try:
        first = s.solve(metrics=True)
        if part == "weight":
            s.set_marker_values(obs_weight=p2.obs_weight)
        else:
            s.set_marker_values(obs_xy=p2.obs_xy)
        second = s.solve(metrics=True)
    finally:
        s.close()
    assert_same_solve(second, fresh_solve(p2, opt, gpu_ctx))
    assert not np.array_equal(first.fvec, second.fvec)


@pytest.mark.parametrize("bad", [0.0, float("nan")])
def test_bad_weight_is_refused_and_changes_nothing(bad, gpu_ctx):
    prob, opt = SCENES["bundles_band"]()
    p2 = perturbed(prob, 11)
    w = p2.obs_weight.copy()
    w[-1] = bad  # the last entry: everything before it is valid
    s = Solver(prob, opt, context=gpu_ctx)
    try:
        before = s.solve(metrics=True)
        with pytest.raises(MmbaError) as e:
            s.set_marker_values(p2.obs_xy, w, None)
        assert e.value.code == abi.MMBA_ERR_INVALID
        s.outputs()  # not even the previous solve's outputs were dropped
        after = s.solve(metrics=True)
    finally:
        s.close()
    assert_same_solve(after, before)


def test_b4_obs_xy_without_frame_xy_is_refused(gpu_ctx):
    prob, opt = SCENES["b4_frame_xy"]()
    p2 = perturbed(prob, 12)
    s = Solver(prob, opt, context=gpu_ctx)
    try:
        before = s.solve(metrics=True)
        with pytest.raises(MmbaError) as e:
            s.set_marker_values(obs_xy=p2.obs_xy)
        assert e.value.code == abi.MMBA_ERR_INVALID
        assert "stale" in str(e.value)
        assert_same_solve(s.solve(metrics=True), before)
        s.set_marker_values()  # nothing given: nothing done
        s.outputs()
    finally:
        s.close()


@pytest.mark.parametrize("name", ["bundles_band", "rolling_shutter", "b4_frame_xy"])
def test_round_trip(name, gpu_ctx):
    prob, opt = SCENES[name]()
    p2 = perturbed(prob, 13)
    s = Solver(prob, opt, context=gpu_ctx)
    try:
        first = s.solve(metrics=True)
        refresh(s, p2)
        moved = s.solve(metrics=True)
        refresh(s, prob)
        back = s.solve(metrics=True)
    finally:
        s.close()
    assert_same_solve(back, first)
    assert not np.array_equal(moved.fvec, first.fvec)
