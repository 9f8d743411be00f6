"""Bounded, offset and scaled parameters, CPU side: the scenes of
tests/test_gpu_bounds.py (synthetic.with_bounds twins of scenes the suite
solves unbounded) and what makes them fit to hold the device to the oracle:

  kinds     every parameter class present (synthetic.param_classes) holds each
            of unbounded / lower-only / upper-only / both -- as many distinct
            kinds as it has parameters where it has fewer than four (the two
            global lens coefficients of the C5 scenes) -- and a scaled and an
            offset parameter;
  flips     at least 10 % of the columns take a negative lmder difference step
            at x0 (synthetic.flipped_columns, adjust_solveFunc.cpp:148-180);
  frozen    every lower-only parameter returns exactly param_min from the
            oracle's solve, with an exactly zero Jacobian column (Appendix B2);
  envelope  the oracle's own x under a 1-ulp change of x0 -- x solved from x0
            against x solved from nextafter(x0), in external values, relative
            to 1 + |x| -- is at most 1e-7, a tenth of the 1e-6 parity bar, so
            a device mismatch cannot be the oracle's own instability; the same
            in the measure the device's x is held in (internal values,
            relative to max(|x|, 1e-3)), and no ||f|| of the trace above 1e8
            times the first (a trial point may overshoot; 1e100 is a wrecked
            scene).

tools/bounds_envelope.py records the envelopes
(profiles/r14_bounds/bounds_envelope.txt)."""
import functools

import numpy as np
import pytest

from mayamatchmovesolver_amd import abi, make_options, synthetic as S

DAG, MMSG = abi.SCENE_GRAPH_MODE_MAYA_DAG, abi.SCENE_GRAPH_MODE_MM_SCENE_GRAPH
LMDER, LMDIF = abi.SOLVER_TYPE_CMINPACK_LMDER, abi.SOLVER_TYPE_CMINPACK_LMDIF
CENTRAL = abi.AUTO_DIFF_TYPE_CENTRAL
ENVELOPE_BAR = 1e-7
MIN_FLIPPED = 0.10


# name: (factory of the unbounded scene, with_bounds seed)
SCENES = {
    "c4_f8": (lambda: S.make_config(3, frames=8, scale=0.001), 8),
    "c2_f6": (lambda: S.make_config(1, frames=6, scale=0.02), 28),
    "c5_f6": (lambda: S.make_config(4, frames=6, scale=0.02), 10),
    "c5_f6_1cam_animated": (lambda: S.make_config(4, frames=6, scale=0.02, cameras=1,
                                                  lens_model="classic_animated"), 27),
    "witness_g4": (lambda: S.witness_scene(n_witness=1, n_focal=1), 8),
    "object": (lambda: S.object_scene(), 38),
    "rig_rows": (lambda: S.rig_scene(stiffness=True), 35),
    "edge": (lambda: S.edge_scene(), 5),
    "edge_parented": (lambda: S.edge_scene(parented=True, solve_bundles=True), 5),
    "rs_f8": (lambda: S.make_config(4, frames=8, scale=0.05, rolling_shutter=0.5), 18),
    "c3_f4": (lambda: S.make_config(2, frames=4, scale=0.002), 7),
    "c4_f40": (lambda: S.make_config(3, frames=40, scale=0.004), 3),
    "c4_f257": (lambda: S.make_config(3, frames=257, scale=0.05), 1),
}


def _cfg(name, **kw):
    return lambda: S.config_options(scene(name), **kw)


# case: (scene, options factory).  The whole solves the GPU module runs.
SOLVES = {
    "c4_f8-mmsg": ("c4_f8", _cfg("c4_f8", iterations=12)),
    "c4_f8-dag": ("c4_f8", _cfg("c4_f8", iterations=12, scene_graph_mode=DAG)),
    "c4_f8-it8": ("c4_f8", _cfg("c4_f8", iterations=8)),
    "c4_f8-lmdif": ("c4_f8", lambda: S.config_options(
        scene("c4_f8"), solver_type=LMDIF, iterations=8 * (scene("c4_f8").num_params + 1) + 6)),
    "c2_f6": ("c2_f6", _cfg("c2_f6")),
    "c2_f6-lmdif": ("c2_f6", _cfg("c2_f6", solver_type=LMDIF)),
    "c5_f6": ("c5_f6", _cfg("c5_f6", iterations=20)),
    "c5_f6_1cam_animated": ("c5_f6_1cam_animated", _cfg("c5_f6_1cam_animated", iterations=20)),
    "witness_g4-dag": ("witness_g4", lambda: make_options(iterations=30)),
    "witness_g4-mmsg": ("witness_g4", lambda: make_options(iterations=30,
                                                           scene_graph_mode=MMSG)),
    "witness_g4-lmdif": ("witness_g4", lambda: make_options(
        solver_type=LMDIF, iterations=4 * (scene("witness_g4").num_params + 1) + 6)),
    "object": ("object", lambda: S.object_options()),
    "object-lmdif": ("object", lambda: S.object_options(solver_type=LMDIF)),
    "rig_rows": ("rig_rows", lambda: make_options(scene_graph_mode=DAG, iterations=30)),
    "edge-central": ("edge", lambda: make_options(auto_diff_type=CENTRAL,
                                                  scene_graph_mode=DAG, iterations=30)),
    "edge_parented": ("edge_parented", lambda: make_options(scene_graph_mode=DAG,
                                                            iterations=30)),
    "rs_f8": ("rs_f8", _cfg("rs_f8", iterations=12)),
    "c3_f4": ("c3_f4", _cfg("c3_f4", iterations=8)),
    "c4_f40": ("c4_f40", _cfg("c4_f40", iterations=6)),
}


@functools.lru_cache(maxsize=None)
def scene(name):
    """The bounded twin of SCENES[name]."""
    make, seed = SCENES[name]
    return S.with_bounds(make(), seed=seed)


def options(case):
    return SOLVES[case][1]()


@functools.lru_cache(maxsize=None)
def oracle_solve(case):
    from oracle import refcpu
    return refcpu.solve(scene(SOLVES[case][0]), options(case))


def envelope(prob, opt, x=None):
    """x' solved from nextafter(x0) against x solved from x0, in two measures:
    max |ext(x') - ext(x)| / (1 + |ext(x)|) in external values, and in the
    measure the device's x is held in (test_gpu_parity.check_solve),
    max |x' - x| / max(|x|, 1e-3) in internal values.  The second is the
    sharper: an upper-only parameter that walks to its bound ends near
    internal 0, where the external value is flat in it."""
    from oracle import refcpu
    if x is None:
        x = refcpu.solve(prob, opt)[0]
    xp = refcpu.solve(prob, opt, x0=np.nextafter(prob.x0, np.inf))[0]
    e, ep = prob.external_params(x), prob.external_params(xp)
    return (float(np.max(np.abs(ep - e) / (1.0 + np.abs(e)))),
            float(np.max(np.abs(xp - x) / np.maximum(np.abs(x), 1e-3))))


@pytest.mark.parametrize("name", sorted(SCENES))
def test_kinds_in_every_class(name):
    prob = scene(name)
    cls, kind = S.param_classes(prob), S.bound_kinds(prob)
    for c in sorted(set(cls.tolist())):
        sel = cls == c
        want = min(4, int(sel.sum()))
        assert len(set(kind[sel].tolist())) >= want, (c, np.bincount(kind[sel], minlength=4))
        if sel.sum() >= 4:
            assert np.any(prob.param_scale[sel] != 1.0) and np.any(prob.param_offset[sel] != 0.0)
    # what the unbounded twin had: none of this
    base = SCENES[name][0]()
    assert not np.any(S.bound_kinds(base)) and np.all(base.param_scale == 1.0)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_flipped_columns(name):
    prob = scene(name)
    fl = S.flipped_columns(prob, 1e-4)
    print("%-22s n %5d flipped %4d" % (name, prob.num_params, int(fl.sum())))
    assert fl.sum() >= MIN_FLIPPED * prob.num_params, (int(fl.sum()), prob.num_params)


def test_central_scene_has_every_delta_pair():
    """Central differences on the bounded edge scene (calculateParameterDelta
    with sign +1 and -1): columns differenced both ways, columns whose two
    deltas coincide at -delta (forward, negative step) and at +delta."""
    prob, d = scene("edge"), 1e-4
    up = (prob.x0 + d) > prob.param_max
    lo = (prob.x0 - d) < prob.param_min
    sa = np.where(lo, 1, np.where(up, -1, 1))
    sb = np.where(lo, 1, np.where(up, -1, -1))
    assert np.any((sa == 1) & (sb == -1))
    assert np.any((sa == -1) & (sb == -1))
    assert np.any((sa == 1) & (sb == 1))


@pytest.mark.parametrize("name", ["c4_f8", "rig_rows"])
def test_lower_only_frozen_in_the_oracle(name, oracle):
    prob = scene(name)
    opt = options({"c4_f8": "c4_f8-mmsg"}.get(name, name))
    frozen = S.bound_kinds(prob) == 1
    assert frozen.any()
    _, J = oracle.jacobian(prob, opt, prob.x0)
    assert not np.any(J[:, frozen]) and np.any(J[:, ~frozen])
    x = oracle.solve(prob, opt)[0]
    np.testing.assert_array_equal(prob.external_params(x)[frozen], prob.param_min[frozen])
    fl = S.flipped_columns(prob, 1e-4) & ~frozen
    assert np.any(J[:, fl])


def test_rig_stiffness_row_on_a_flipped_bounded_parameter():
    prob = scene("rig_rows")
    hit = np.isin(prob.param_attr, np.concatenate([prob.stiff_attr, prob.smooth_attr]))
    fl = S.flipped_columns(prob, 1e-4) & (S.bound_kinds(prob) >= 2)
    assert np.any(hit & fl), (S.bound_kinds(prob)[hit], fl[hit])


@pytest.mark.parametrize("case", sorted(SOLVES))
def test_oracle_envelope(case, oracle):
    prob, opt = scene(SOLVES[case][0]), options(case)
    x, _f, _eu, _ed, res, trace = oracle_solve(case)
    env = envelope(prob, opt, x)
    print("%-22s n %4d reason %d evals %4d ||f|| %.6e -> %.6e envelope %.1e external, %.1e "
          "internal" % (case, prob.num_params, res.reason_number, res.function_evals, trace[0],
                        trace[-1], env[0], env[1]))
    # a scene the bounds have not wrecked: no trial point blows ||f|| up
    assert np.all(np.isfinite(x)) and np.max(trace) <= 1e8 * trace[0]
    assert max(env) <= ENVELOPE_BAR, env


def test_per_frame_envelope(oracle):
    """The per-frame solve of the bounded C2 scene (frame by frame, x carried
    along) under the same 1-ulp change of x0, in both measures."""
    from tests.test_gpu_perframe import oracle_per_frame
    prob, opt = scene("c2_f6"), options("c2_f6")
    x, rr = oracle_per_frame(prob, opt, oracle)
    xp, _rr = oracle_per_frame(prob.with_x0(np.nextafter(prob.x0, np.inf)), opt, oracle)
    assert len(rr) == prob.num_frames
    e, ep = prob.external_params(x), prob.external_params(xp)
    env = (float(np.max(np.abs(ep - e) / (1.0 + np.abs(e)))),
           float(np.max(np.abs(xp - x) / np.maximum(np.abs(x), 1e-3))))
    print("c2_f6 per frame        envelope %.1e external, %.1e internal" % env)
    assert max(env) <= ENVELOPE_BAR, env
