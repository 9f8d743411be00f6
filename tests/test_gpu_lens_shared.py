"""An animated lens coefficient shared by several cameras, at any frame count.

Two (or three) cameras on one 3DE-classic lens with its distortion keyed per
frame: a frame's coefficient is read by the rows of every camera at that
frame, so it used to be one global parameter per frame and the plan was
refused beyond NGMAX = 48 frames.  The shared form (Plan::build,
mmba_lens_shared.hip, MMBA_PATH_LENS_SHARED) hosts the coefficient in the
block of the frame's first reading camera-frame; the other cameras' rows carry
its column beside their own block's and couple their camera-frame to the
host's through an off-diagonal block of the band.

Scenes: S.make_config(4, frames=F, scale=s, lens_model="classic_animated",
cameras=c) with S.config_options.  By default the shared form is taken only
where the global form exceeds NGMAX (F = 50); on the small scenes it is pinned
on.

Bars.  f at 1e-12 and J at 1e-7 of its largest entry with the same zero
pattern (tests/test_gpu_lens_cf.py).  The damped step, g and D at the bars of
tests/test_gpu_damped_step.py (1000 e64 on the device's J; a pair is
admissible when 1000 e64 <= 1e-7 on the oracle's J, asserted on the CPU by
test_step_scenes_admissible together with the one-observation mutation; no
pair had to be left out).  Whole solves through check_solve at 1e-6 (reason,
counts, every ||f|| of the trace, x).  The oracle's own 1-ulp envelope of x
over the 8 registered seeds of tests/golden/envelopes.py (from the oracle
alone) is 3.4e-9 on the 6-frame scene and 1.3e-7 on the 50-frame one, below
1e-6 on both, so x is held whole, not in a determined subspace.

The 50-frame whole solve runs at scale 0.08 (7,933 observations), against a
fixture (tests/golden/make_lens_shared.py): the oracle's run takes over a
minute, 651 FD columns per outer iteration.  At scale 0.05, the scene of the
structure, Jacobian and step tests, the reference's run is not determined at
the trace bar: its third and fourth evaluations are rejected wild trial
points (||f|| = 7.7e265, then 7.3e3 from 3.6e3) where the oracle's own ||f||
moves by 9e-4 and 7e-3 under a 1-ulp change of x0 (seeds 1000-1002; every
other evaluation by less than 2e-8).  The device's run of that scene agrees
with the oracle's in reason, counts and final x (7.9e-9 against an envelope
of 5.6e-7) and in the trace at 1e-6 except at those two evaluations (inf,
where the plain sum of squares overflows and MINPACK's enorm does not, and
8.8e-5, inside the oracle's own spread).  At scale 0.08 the run has 16
evaluations and the oracle's ||f|| moves by less than 7e-10 at every one.

Measured on an MI355X, e64 / the device's error of the step (on the device's
J; every run prints these lines with -s; g and D stayed below 6e-4 of their
bars):

scene        n      m  lam 1              lam 1e-3           lam 0
f6_c2       79   1200  1.0e-15 / 6.9e-16  2.8e-15 / 1.5e-15  2.5e-15 / 1.2e-15
f6_c3      115   1440  1.2e-15 / 8.9e-16  2.5e-15 / 3.5e-15  3.1e-15 / 2.7e-15
f50_c2     651   9928  1.0e-14 / 9.0e-16  1.7e-14 / 2.5e-15  1.3e-14 / 2.4e-15

The largest device error is 1.4 x e64 (f6_c3 at lam = 1e-3), against the
margin of 1000.
"""
import functools

import numpy as np
import pytest

from mayamatchmovesolver_amd import abi, synthetic as S
from mayamatchmovesolver_amd._lib import MmbaError
from mayamatchmovesolver_amd.solver import Solver
from tests.test_gpu_damped_step import (EPS, LAMS, SIGN, STEP_CAP, STEP_CAP_DEVICE, Reference,
                                        step_error)

gpu = pytest.mark.gpu

# name: (frames, scale, cameras, MMBA_PATH_LENS_SHARED pin or None)
SCENES = {
    "f6_c2": (6, 0.05, 2, 1),
    "f6_c3": (6, 0.06, 3, 1),
    "f50_c2": (50, 0.05, 2, None),
    "f50_c3": (50, 0.1, 3, None),
}
STEP_SCENES = ["f6_c2", "f6_c3", "f50_c2"]
# (scene, lam) pairs with 1000 e64 > 1e-7 on the oracle's J: none
LEFT_OUT = {}


@functools.lru_cache(maxsize=None)
def scene(name):
    F, s, c, _pin = SCENES[name]
    return S.make_config(4, frames=F, scale=s, lens_model="classic_animated", cameras=c)


def build(name, ctx, paths):
    """The scene's plan, MMBA_PATH_LENS_SHARED pinned as the table says."""
    pin = SCENES[name][3]
    if pin is not None:
        paths(abi.PATH_LENS_SHARED, pin)
    prob = scene(name)
    return prob, S.config_options(prob), Solver(prob, S.config_options(prob), context=ctx)


def frame_coefficients(prob):
    """The per-frame lens coefficients (parameter ids)."""
    lens = set(int(a) for a in np.asarray(prob.lens_attrs).ravel() if a >= 0)
    return [p for p in range(prob.num_params)
            if prob.param_frame[p] >= 0 and int(prob.param_attr[p]) in lens]


def assert_coupled(prob, J):
    """Every per-frame coefficient has non-zero rows on at least two cameras,
    all at its own frame: the scene exercises the coupling."""
    cam = np.asarray(prob.mkr_cam)[prob.obs_marker]
    coefs = frame_coefficients(prob)
    assert len(coefs) == prob.num_frames
    for p in coefs:
        rows = np.flatnonzero(J[:, p] != 0.) // 2
        assert rows.size > 0
        assert np.all(prob.obs_frame[rows] == prob.param_frame[p]), p
        assert len(set(cam[rows].tolist())) >= 2, (p, set(cam[rows].tolist()))


@functools.lru_cache(maxsize=None)
def oracle_jacobian(name, shift):
    from oracle import refcpu
    prob = scene(name)
    f, J = refcpu.jacobian(prob, S.config_options(prob), prob.x0 + shift)
    return f, np.ascontiguousarray(J)


# ---- CPU: the step scenes are admissible and can notice an error ----

def without_observation(ref, J, f, i):
    """The Reference of J with observation i's two rows zeroed, by a rank-two
    downdate of ref's sums (the same sums Reference forms from the zeroed J,
    up to the order of the extended-precision additions)."""
    Ji, fi = J[2 * i:2 * i + 2], f[2 * i:2 * i + 2]
    Jl = Ji.astype(np.longdouble)
    r = object.__new__(Reference)
    r.m = ref.m
    r.A = ref.A - Jl.T @ Jl
    r.g = ref.g - SIGN * (Jl.T @ fi.astype(np.longdouble))
    r.abs_g = ref.abs_g - np.abs(Ji).T @ np.abs(fi)
    d2 = np.diagonal(r.A).copy()
    r.D = np.sqrt(np.maximum(d2, 0))
    r.D[d2 <= 0] = 1.0
    r.A64 = ref.A64 - Ji.T @ Ji
    r.g64 = ref.g64 - SIGN * (Ji.T @ fi)
    D64 = np.sqrt(np.maximum(np.diagonal(r.A64), 0.))
    D64[D64 == 0.] = 1.0
    r.D64 = D64
    r._steps = {}
    return r


@pytest.mark.parametrize("name", STEP_SCENES)
def test_step_scenes_admissible(name):
    """On the oracle's J at x0 (as test_one_observation_moves_the_reference):
    every (scene, lam) pair tested has 1000 e64 <= 1e-7, lam = 1 and 1e-3
    remain for every scene, and zeroing one observation's two rows (the
    first, the middle and the last live one, each alone) moves the reference
    step by at least 1000 x the step bar.  The oracle's J shows the coupling."""
    prob = scene(name)
    f, J = oracle_jacobian(name, 0.0)
    assert_coupled(prob, J)
    ref = Reference(J, f)
    live = [i for i in range(prob.num_obs) if np.any(J[2 * i:2 * i + 2] != 0.)]
    lams = [lam for lam in LAMS if (name, lam) not in LEFT_OUT]
    assert 1.0 in lams and 1e-3 in lams
    muts = [without_observation(ref, J, f, i) for i in (live[0], live[len(live) // 2], live[-1])]
    for lam in LAMS:
        p_ref, e64 = ref.step(lam)
        moved = min(step_error(rz.step(lam)[0], p_ref, ref.D.astype(np.float64)) for rz in muts)
        print("%-8s lam %-6g n %4d  e64 %.2g  bar %.2g  one observation moves the step by >= %.2g"
              % (name, lam, J.shape[1], e64, ref.step_bar(lam), moved))
        if lam in lams:
            assert ref.step_bar(lam) <= STEP_CAP, (lam, e64)
            assert moved >= 1000.0 * ref.step_bar(lam), (lam, moved)
        else:
            assert ref.step_bar(lam) > STEP_CAP, (lam, e64)


# ---- GPU ----

@gpu
@pytest.mark.parametrize("name,dim", [("f50_c2", 50 * 13 + 1), ("f50_c3", 50 * 19 + 1)])
def test_plan_builds_beyond_the_cap(name, dim, gpu_ctx, paths):
    """50 frames: the global form would hold 50 + 1 globals and was refused
    ("more than 48 global parameters").  The plan builds, every frame's
    coefficient sits in a camera-frame block (13 = 7 + 6 rows per frame with
    two cameras, 19 with three), the static quartic is the one global, and the
    reduced system is a band the log-depth solver or the band chain takes."""
    prob, _opt, s = build(name, gpu_ctx, paths)
    try:
        if name == "f50_c2":
            assert prob.num_params == 651 and prob.num_obs == 4964
        st = s.kernel_stats()
        assert st["reduced_dim"] == dim, st
        assert st["reduced_kind"] == 0, st
        assert st["band_solver"] in (1, 2), st
    finally:
        s.close()


@gpu
@pytest.mark.parametrize("name", ["f50_c2", "f6_c2"])
def test_residuals_and_jacobian(name, oracle, gpu_ctx, paths):
    prob, opt, s = build(name, gpu_ctx, paths)
    try:
        x1 = prob.x0 + 0.01
        f1, _, _, _ = s.measure(x1)
        f1_ref, _, _, _ = oracle.measure(prob, opt, x1)
        np.testing.assert_allclose(f1, f1_ref, rtol=1e-12, atol=1e-12)
        J = s.jacobian(x1)
        _f, J_ref = oracle_jacobian(name, 0.01)
        assert_coupled(prob, J_ref)
        scale = np.max(np.abs(J_ref))
        assert np.max(np.abs(J - J_ref)) <= 1e-7 * scale
        assert np.array_equal(J != 0, J_ref != 0) or np.max(np.abs(J[J_ref == 0])) < 1e-9 * scale
    finally:
        s.close()


_runs = {}


def device_run(name, ctx, paths):
    """One plan of the scene: the damped step at x0 for every lam, twice, the
    dense J of the pass, f, and the reference built from the device's J, f."""
    if name in _runs:
        return _runs[name]
    prob, _opt, s = build(name, ctx, paths)
    try:
        st = s.kernel_stats()
        out, again, J0 = {}, {}, None
        for lam in LAMS:
            step, g, diag, J = s.damped_step(prob.x0, lam)
            if J0 is None:
                J0 = J
            else:
                np.testing.assert_array_equal(J, J0)
            out[lam] = (step, g, diag)
        for lam in LAMS:
            again[lam] = s.damped_step(prob.x0, lam, jacobian=False)[:3]
        f = s.measure(prob.x0)[0]
    finally:
        s.close()
    _runs[name] = dict(stats=st, out=out, again=again, J=J0, f=f, ref=Reference(J0, f))
    return _runs[name]


@gpu
@pytest.mark.parametrize("name,lam", [pytest.param(n, lam, id="%s-lam%g" % (n, lam))
                                      for n in STEP_SCENES for lam in LAMS
                                      if (n, lam) not in LEFT_OUT])
def test_damped_step(name, lam, gpu_ctx, paths):
    """g, D and the damped step against the extended-precision reference of
    the device's own J and f (tests/test_gpu_damped_step.py's bars)."""
    run = device_run(name, gpu_ctx, paths)
    st, ref = run["stats"], run["ref"]
    assert st["reduced_kind"] == 0 and st["band_solver"] in (1, 2), st
    assert st["reduced_dim"] == scene(name).num_params, st  # no solved bundle
    step, g, diag = run["out"][lam]
    p_ref, e64 = ref.step(lam)
    D = ref.D.astype(np.float64)
    m = ref.m
    g_ref = ref.g.astype(np.float64)
    g_bar = 4.0 * m * EPS * ref.abs_g
    g_err = float(np.max(np.abs(g - g_ref) / np.maximum(g_bar, np.finfo(float).tiny)))
    d_err = float(np.max(np.abs(diag - D) / (4.0 * m * EPS * D)))
    err = step_error(step, p_ref, D)
    print("%-8s lam %-6g n %4d m %6d  e64 %.2g  bar %.2g  device %.2g  (g %.2g, D %.2g of their "
          "bars)" % (name, lam, D.size, m, e64, ref.step_bar(lam), err, g_err, d_err))
    assert np.all(np.isfinite(step)) and np.all(np.isfinite(g)) and np.all(np.isfinite(diag))
    assert ref.step_bar(lam) <= STEP_CAP_DEVICE, "no sharp bar on this J: e64 %.3g" % e64
    assert np.all(np.abs(g - g_ref) <= g_bar), "g: %.3g of its bar" % g_err
    assert np.all(np.abs(diag - D) <= 4.0 * m * EPS * D), "D: %.3g of its bar" % d_err
    assert err <= ref.step_bar(lam), "step: %.3g against %.3g" % (err, ref.step_bar(lam))


@gpu
@pytest.mark.parametrize("name", STEP_SCENES)
def test_damped_step_repeats_bit_for_bit(name, gpu_ctx, paths):
    """Two damped_step calls on one plan return identical arrays (fixed
    summation order, no atomics in the shared form's kernels)."""
    run = device_run(name, gpu_ctx, paths)
    for lam in LAMS:
        for a, b, what in zip(run["out"][lam], run["again"][lam], ("step", "g", "D")):
            np.testing.assert_array_equal(a, b, err_msg="%s at lam %g" % (what, lam))


@gpu
@pytest.mark.parametrize("shared", [1, 0])
def test_two_forms_one_scene(shared, oracle, gpu_ctx, paths):
    """6 frames, two cameras: the shared form and the global form (today's
    path) each against the oracle -- reason, counts, every ||f|| of the trace
    and x at 1e-6 (the oracle's 1-ulp envelope of this x is 3.4e-9)."""
    from tests.test_gpu_parity import check_solve
    paths(abi.PATH_LENS_SHARED, shared)
    prob = scene("f6_c2")
    seen = {}

    def run(s):
        seen.update(s.kernel_stats())
        return s.solve()
    check_solve(prob, S.config_options(prob), oracle, gpu_ctx, run=run)
    # shared: 6 x (7 + 6) block rows and the quartic; global: 6 x 12 and 6 + 1 globals
    assert seen["reduced_dim"] == prob.num_params
    assert seen["reduced_kind"] == (0 if shared else 3), seen


class FixtureOracle:
    """check_solve's oracle, answering from a fixture of
    tests/golden/make_lens_shared.py (the oracle's run of the 50-frame scene
    takes minutes: n FD columns per outer iteration)."""

    class Result:
        def __init__(self, d):
            self._d = {k[4:]: v.item() for k, v in d.items() if k.startswith("res_")}
            self.__dict__.update(self._d)

        def as_dict(self):
            return dict(self._d)

    def __init__(self, d):
        self.d = d

    def solve(self, prob, opt):
        d = self.d
        return d["exp_x"], d["exp_fvec"], None, None, self.Result(d), d["exp_trace"]


def test_whole_solve_fixture():
    """The fixture is the oracle's run of the scene as generated now, and its
    envelope -- the registered seeds -- lies below the 1e-6 bar: x is held
    whole."""
    from tests.golden import make_lens_shared as LS
    from tests.golden.envelopes import SEEDS
    prob, _opt, d = LS.load("c5_f50_lens_anim_2cam")  # raises on a digest mismatch
    assert prob.num_frames == 50 and prob.num_cameras == 2 and prob.num_params == 651
    assert tuple(d["envelope_seeds"]) == SEEDS and int(d["envelope_runs"]) == len(SEEDS)
    assert float(d["exp_x_envelope"]) <= 1e-6
    assert d["exp_x"].size == prob.num_params and d["exp_fvec"].size == prob.num_residuals
    assert d["exp_trace"].size == int(d["res_function_evals"])
    assert abs(np.linalg.norm(d["exp_fvec"]) - float(d["res_error_final"])) <= \
        1e-12 * float(d["res_error_final"])


@gpu
def test_whole_solve_beyond_the_cap(gpu_ctx, paths):
    """50 frames, two cameras (scale 0.08: the module docstring says why),
    through check_solve at 1e-6 against the oracle's fixture; the plan is the
    shared form's, by default."""
    from tests.golden import make_lens_shared as LS
    from tests.test_gpu_parity import check_solve
    prob, opt, d = LS.load("c5_f50_lens_anim_2cam")
    seen = {}

    def run(s):
        seen.update(s.kernel_stats())
        return s.solve()
    check_solve(prob, opt, FixtureOracle(d), gpu_ctx, run=run)
    assert seen["reduced_dim"] == 50 * 13 + 1 and seen["reduced_kind"] == 0, seen


@gpu
@pytest.mark.parametrize("key,why", [(abi.PATH_LENS_SHARED, "MMBA_PATH_LENS_SHARED = 0"),
                                     (abi.PATH_LENS_CF, "MMBA_PATH_LENS_CF = 0")])
def test_pinned_off_keeps_the_refusal(key, why, gpu_ctx, paths):
    """Either pin at 0: every frame's coefficient a global again, 50 + 1 >
    NGMAX, refused as before, and the message names the pin."""
    paths(key, 0)
    prob = scene("f50_c2")
    with pytest.raises(MmbaError) as e:
        Solver(prob, S.config_options(prob), context=gpu_ctx).close()
    assert "48 global" in str(e.value)
    assert why in str(e.value)
