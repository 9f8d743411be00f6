"""Per-frame object tracking, host side: the cases of
tests/test_gpu_perframe_object.py run through the CPU oracle frame by frame
(tests.test_gpu_perframe.oracle_per_frame), so the GPU file holds the one
launch to references that are known to be sound.

Per case: the oracle solves every frame, every parameter is keyed at one
frame, and the per-frame parameter counts are the ones the batched kernel's
instantiations are chosen by.  The bounded twins must really flip difference
signs and hold frames that are written back and frames that are not; the blind
frame of ``windows`` must end after one evaluation.  The oracle's own x
envelope on every case is in profiles/r15_perframe_object/envelope.txt
(tools/perframe_object_envelope.py; all below the 1e-7 a case may have under
the 1e-6 bar)."""
import numpy as np
import pytest

from mayamatchmovesolver_amd import abi, synthetic as S
from tests.test_gpu_perframe import frame_params_only, oracle_per_frame

DAG, MMSG = abi.SCENE_GRAPH_MODE_MAYA_DAG, abi.SCENE_GRAPH_MODE_MM_SCENE_GRAPH
LMDER, LMDIF = abi.SOLVER_TYPE_CMINPACK_LMDER, abi.SOLVER_TYPE_CMINPACK_LMDIF


def _small():
    return S.object_scene(frames=3, bundles=6)


def _above_cap():
    return S.object_scene(**S.OBJECT_TEST_SCENES["above_cap"])


def _four():
    return S.object_scene(frames=4, bundles=6)


def _weighted():
    prob = _four()
    prob.param_weight = np.linspace(0.5, 2.0, prob.num_params)
    return prob


# name -> (scene, options keywords, parameters per frame, interrupt_after)
CASES = {}
for _m, _mn in ((DAG, "dag"), (MMSG, "mmsg")):
    for _s, _sn in ((LMDER, "lmder"), (LMDIF, "lmdif")):
        _kw = dict(scene_graph_mode=_m, solver_type=_s)
        CASES["small-%s-%s" % (_mn, _sn)] = (_small, _kw, [6] * 3, -1)
        CASES["above_cap-%s-%s" % (_mn, _sn)] = (_above_cap, _kw, [6] * 9, -1)
CASES.update({
    "parent": (lambda: S.object_scene(**S.OBJECT_TEST_SCENES["parent"]), {}, [6] * 9, -1),
    "windows": (lambda: S.object_scene(**S.OBJECT_TEST_SCENES["windows"]), {}, [6] * 10, -1),
    "two_objects": (lambda: S.object_scene(frames=5, bundles=6, objects=2), {}, [12] * 5, -1),
    "camera_object-lmder": (
        lambda: frame_params_only(S.object_scene(frames=5, bundles=6, solve_camera=True)),
        dict(solver_type=LMDER), [6, 12, 12, 12, 12], -1),
    "camera_object-lmdif": (
        lambda: frame_params_only(S.object_scene(frames=5, bundles=6, solve_camera=True)),
        dict(solver_type=LMDIF), [6, 12, 12, 12, 12], -1),
    "many_rows": (lambda: S.object_scene(frames=3, bundles=260), {}, [6] * 3, -1),
    "bounded_small": (lambda: S.with_bounds(_small(), seed=1), {}, [6] * 3, -1),
    "bounded_above_cap": (lambda: S.with_bounds(_above_cap(), seed=0), {}, [6] * 9, -1),
    "opt-no_accept_only_better": (_four, dict(accept_only_better=0), [6] * 4, -1),
    "opt-maxfev": (_four, dict(iterations=3), [6] * 4, -1),
    "opt-initial_error_given": (_four, dict(initial_error_avg=1e6), [6] * 4, -1),
    "opt-param_weights": (_weighted, dict(auto_param_scale=0), [6] * 4, -1),
    "interrupt_pending": (_four, {}, [6] * 4, 0),
})

_cache = {}


def case(name, oracle):
    """(problem, options, oracle x, oracle per-frame results) of a case,
    computed once per session and shared by both test files."""
    if name not in _cache:
        build, kw, _sizes, after = CASES[name]
        prob = build()
        opt = S.object_options(**kw)
        xr, rr = oracle_per_frame(prob, opt, oracle, interrupt_after=after)
        xr.setflags(write=False)
        _cache[name] = (prob, opt, xr, rr)
    return _cache[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_solves_every_frame(name, oracle):
    prob, _opt, _xr, rr = case(name, oracle)
    sizes = CASES[name][2]
    assert np.all(np.asarray(prob.param_frame) >= 0)
    assert np.bincount(prob.param_frame, minlength=prob.num_frames).tolist() == sizes
    assert len(rr) == prob.num_frames
    for f, r in enumerate(rr):
        assert r.success == 1, (f, r.as_dict())
        if CASES[name][3] < 0:
            assert r.reason_number > 0, (f, r.as_dict())
        else:
            assert r.reason_number == -1 and r.user_interrupted == 1, (f, r.as_dict())


@pytest.mark.parametrize("name", ["bounded_small", "bounded_above_cap"])
def test_bounded_twins_flip_and_mix(name, oracle):
    prob, opt, _xr, rr = case(name, oracle)
    assert np.mean(S.flipped_columns(prob, opt.delta)) >= 0.10
    better = [r.error_is_better for r in rr]
    assert 0 in better and 1 in better, better


def test_per_frame_plan_is_unsharded():
    """Solver(per_frame=True) with a communicator raises before any device call."""
    from mayamatchmovesolver_amd.solver import Solver
    with pytest.raises(ValueError):
        Solver(_small(), S.object_options(), comm=object(), per_frame=True)


def test_bindings_list_the_new_entry_points():
    assert "mmba_plan_create_per_frame" in abi.EXPORTED_SYMBOLS
    assert "mmba_debug_batch_launches" in abi.EXPORTED_SYMBOLS


def test_blind_frame_ends_after_one_evaluation(oracle):
    _prob, _opt, _xr, rr = case("windows", oracle)
    blind = rr[-1]
    assert blind.function_evals == 1 and blind.iterations == 1, blind.as_dict()
    assert blind.error_is_better == 1
