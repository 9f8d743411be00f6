"""Bounded, offset and scaled parameters on the device against the oracle.

The box-constraint reparametrisation (adjust_base.cpp:194-258) and the
bound-dependent difference sign (adjust_solveFunc.cpp:148-180) are applied in
five separately written places on the device ("Bounded
parameters").  Every scene here is the synthetic.with_bounds twin of a scene
the suite solves unbounded: each parameter class holds every kind of bound, a
scaled and an offset parameter, a tenth or more of the columns take a negative
difference step at x0, and the oracle's own 1-ulp envelope is below 1e-7
(tests/test_bounds_host.py), so a mis-indexed or mis-permuted p_min / p_max /
p_off / p_scale, a dropped sign or a scale read as 1 shows as a mismatch.

Bars.  measure 1e-12; the FD Jacobian 1e-7 of the oracle's largest entry;
the whole solve at test_gpu_parity.py's bars (x and every ||f|| 1e-6, reason
and counts equal).  g = J^T f and D = ||J col|| of mmba_debug_damped_step are
held twice: to the extended-precision reference of the call's own J at the
bars of test_gpu_damped_step.py, and to the oracle's J and f at what the
Jacobian's bar allows -- with |J - J_ref| <= t = 1e-7 max|J_ref| per entry,
|g - g_ref| <= t ||f||_1 and |D - D_ref| <= t sqrt(m) (triangle inequality),
plus the 4 m eps rounding bars of the first comparison.

Which path ran is read from the plan: mmba_plan_param_layout (lens and object
parameters in camera-frame blocks), mmba_plan_num_shards, and
mmba_kernel_stats (reduced_kind, trial_red_folds).  The per-frame batch and
the (GROUP, ONEPASS) forms leave no statistic: the pins are taken on trust
there, as in test_gpu_perframe.py and test_gpu_backsub_group.py.
"""
import functools

import numpy as np
import pytest

from mayamatchmovesolver_amd import abi, synthetic as S
from mayamatchmovesolver_amd.solver import Context, Solver, shard_layout, solve_per_frame
from tests.test_bounds_host import SOLVES, oracle_solve, options, scene
from tests.test_gpu_backsub_group import FORMS
from tests.test_gpu_damped_step import EPS, STEP_CAP, check_bars
from tests.test_gpu_perframe import check_frames, oracle_per_frame

pytestmark = pytest.mark.gpu

REL = 1e-6
JAC_BAR = 1e-7
LMDER = abi.SOLVER_TYPE_CMINPACK_LMDER
CF, BND, GLOB = 0, 1, 2  # mmba_plan_param_layout's classes
TILED, DENSE = 1, 2      # mmba_kernel_stats.reduced_kind


# ---- the checks ----

def check_whole_solve(case, out):
    """test_gpu_parity.check_solve's assertions on a finished device solve of
    SOLVES[case], and the frozen lower-only parameters exactly at param_min."""
    prob = scene(SOLVES[case][0])
    xr, _fr, _eur, _edr, rr, trr = oracle_solve(case)
    g = out.result
    assert g["reason_number"] == rr.reason_number, (g, rr.as_dict())
    assert g["iterations"] == rr.iterations
    assert g["outer_iterations"] == rr.outer_iterations
    assert g["function_evals"] == rr.function_evals
    assert g["jacobian_evals"] == rr.jacobian_evals
    assert len(out.fnorm_trace) == len(trr)
    err_t = float(np.max(np.abs(out.fnorm_trace - trr) / trr))
    err_x = float(np.max(np.abs(out.x - xr) / np.maximum(np.abs(xr), 1e-3)))
    print("%-24s evals %3d  trace %.2g  x %.2g" % (case, rr.function_evals, err_t, err_x))
    np.testing.assert_allclose(out.fnorm_trace, trr, rtol=REL, atol=1e-9 * trr[0])
    assert err_x <= REL, (out.x, xr)
    assert abs(g["error_final"] - rr.error_final) <= REL * rr.error_final + 1e-9 * trr[0]
    frozen = S.bound_kinds(prob) == 1
    np.testing.assert_array_equal(prob.external_params(out.x)[frozen], prob.param_min[frozen])


def check_jacobian(prob, opt, oracle, J):
    """The device's dense FD Jacobian at x0 against the oracle's: 1e-7 of the
    largest entry, exact zeros where the oracle has them, the frozen columns
    exactly zero, and the columns differenced with a negative step non-zero
    wherever the oracle's are.  Returns the oracle's (f, J)."""
    f_ref, J_ref = oracle.jacobian(prob, opt, prob.x0)
    big = np.max(np.abs(J_ref))
    assert np.max(np.abs(J - J_ref)) <= JAC_BAR * big, np.max(np.abs(J - J_ref)) / big
    assert np.max(np.abs(J[J_ref == 0.])) <= 1e-9 * big
    # frozen columns: exactly zero -- but for the rows an animated central
    # column skips, which hold f_j / (2 (|dA| + |dB|)) in the reference (B15)
    frozen = S.bound_kinds(prob) == 1
    assert frozen.any()
    if opt.auto_diff_type == abi.AUTO_DIFF_TYPE_CENTRAL:
        assert np.array_equal(J[:, frozen] != 0., J_ref[:, frozen] != 0.)
        own = prob.obs_frame[:, None] == prob.param_frame[frozen][None, :]
        assert not np.any(J[:2 * prob.num_obs].reshape(prob.num_obs, 2, -1)[:, :, frozen]
                          [np.broadcast_to(own[:, None, :], (prob.num_obs, 2, own.shape[1]))])
    else:
        assert not np.any(J[:, frozen])
    if opt.solver_type == LMDER:
        fl = S.flipped_columns(prob, opt.delta) & ~frozen
        live = np.any(J_ref[:, fl] != 0., axis=0)
        assert live.sum() >= 0.05 * prob.num_params, (int(live.sum()), prob.num_params)
        assert np.all(J[:, fl][J_ref[:, fl] != 0.] != 0.)
    return f_ref, J_ref


def check_first_iteration(name, prob, opt, oracle, s):
    """measure at x0, then J, g and D of one mmba_debug_damped_step call."""
    f = s.measure(prob.x0)[0]
    f_ref = oracle.measure(prob, opt, prob.x0)[0]
    np.testing.assert_allclose(f, f_ref, rtol=1e-12, atol=1e-12)
    step, g, diag, J = s.damped_step(prob.x0, 1.0)
    _f, J_ref = check_jacobian(prob, opt, oracle, J)
    # against the call's own J (bars of test_gpu_damped_step.py)
    check_bars(name, 1.0, dict(out={1.0: (step, g, diag)}, J=np.ascontiguousarray(J), f=f,
                               ref=None))
    # against the oracle's J and f (module docstring)
    m = J_ref.shape[0]
    t = JAC_BAR * np.max(np.abs(J_ref))
    g_ref = J_ref.T @ f_ref
    D_ref = np.linalg.norm(J_ref, axis=0)
    D_ref[D_ref == 0.] = 1.0
    g_bar = t * np.sum(np.abs(f_ref)) + 4.0 * m * EPS * (np.abs(J_ref).T @ np.abs(f_ref))
    assert np.all(np.abs(g - g_ref) <= g_bar), np.max(np.abs(g - g_ref) / g_bar)
    D_bar = t * np.sqrt(m) + 4.0 * m * EPS * D_ref
    assert np.all(np.abs(diag - D_ref) <= D_bar), np.max(np.abs(diag - D_ref) / D_bar)


def run_case(case, oracle, ctx, first="step", layout=None, stats=None):
    """One plan of SOLVES[case]: the first iteration's pieces against the
    oracle (``first``: "step" through mmba_debug_damped_step, "jacobian"
    through mmba_plan_jacobian where the hook refuses the plan), then the
    whole solve."""
    prob, opt = scene(SOLVES[case][0]), options(case)
    s = Solver(prob, opt, context=ctx)
    try:
        if layout is not None:
            layout(prob, *s.param_layout())
        if stats is not None:
            stats(s)
        if first == "step":
            check_first_iteration(case, prob, opt, oracle, s)
        else:
            f = s.measure(prob.x0)[0]
            np.testing.assert_allclose(f, oracle.measure(prob, opt, prob.x0)[0], rtol=1e-12,
                                       atol=1e-12)
            check_jacobian(prob, opt, oracle, s.jacobian(prob.x0))
        out = s.solve()
    finally:
        s.close()
    check_whole_solve(case, out)
    return out


# ---- a. against the oracle ----

@pytest.mark.parametrize("case", ["c4_f8-mmsg", "c4_f8-dag", "c4_f8-lmdif", "c2_f6", "c2_f6-lmdif",
                                  "witness_g4-dag", "witness_g4-mmsg", "witness_g4-lmdif"])
def test_bounded_twin_matches_oracle(case, oracle, gpu_ctx):
    run_case(case, oracle, gpu_ctx)


def lens_layout(cf):
    def check(prob, cls, blk):
        lens = S.param_classes(prob) == "lens"
        if not lens.any():  # the shared lens' coefficients are static: globals either way
            assert np.all(cls[prob.param_frame < 0] == GLOB)
        else:
            assert np.all(cls[lens] == (CF if cf else GLOB)), cls[lens]
    return check


@pytest.mark.parametrize("lens_cf", [0, 1])
@pytest.mark.parametrize("case", ["c5_f6", "c5_f6_1cam_animated"])
def test_bounded_lens_scene(case, lens_cf, oracle, gpu_ctx, paths):
    """The C5 scene (two cameras, the shared lens' two coefficients global)
    and its one-camera form with the distortion keyed per frame: bounded lens
    coefficients in the global arrow (MMBA_PATH_LENS_CF = 0) and in their
    camera-frame's block (VF_LENS, = 1)."""
    paths(abi.PATH_LENS_CF, lens_cf)
    run_case(case, oracle, gpu_ctx, layout=lens_layout(lens_cf))


@pytest.mark.parametrize("rec", [0, 1])
@pytest.mark.parametrize("case", ["object", "object-lmdif"])
def test_bounded_object_scene(case, rec, oracle, gpu_ctx, paths):
    """Bounded object poses in their camera-frame's block (VF_OBJ,
    MMBA_PATH_OBJ_CF = 1), by the chain walk (MMBA_PATH_OBJ_REC = 0) and by the
    object records (= 1)."""
    paths(abi.PATH_OBJ_CF, 1)
    paths(abi.PATH_OBJ_REC, rec)

    def layout(prob, cls, blk):
        assert np.all(cls == CF) and np.array_equal(blk, prob.param_frame)
    run_case(case, oracle, gpu_ctx, layout=layout)


# ---- b. path coverage at small shapes ----

def test_rig_rows(oracle, gpu_ctx):
    """Every parameter static, a stiffness row on a bounded parameter whose
    difference step is negative (k_rows_jac)."""
    run_case("rig_rows", oracle, gpu_ctx, first="jacobian")


def test_edge_central(oracle, gpu_ctx):
    """Central differences on the bounded edge scene (the animated bundle
    scene of test_gpu_b15.py): k_param_central with columns differenced both
    ways and columns whose two deltas coincide, at -delta and at +delta, which
    stay forward (tests/test_bounds_host.py asserts all three are present)."""
    run_case("edge-central", oracle, gpu_ctx, first="jacobian")


def test_rolling_shutter(oracle, gpu_ctx):
    run_case("rs_f8", oracle, gpu_ctx, first="jacobian")


@pytest.mark.parametrize("dense", [0, 1])
def test_dense_and_tiled(dense, oracle, gpu_ctx, paths):
    paths(abi.PATH_DENSE, dense)

    def stats(s):
        assert s.kernel_stats()["reduced_kind"] == (DENSE if dense else TILED)
    run_case("c3_f4", oracle, gpu_ctx, stats=stats)


@pytest.mark.parametrize("form", ["separator", "whole", "partitioned"])
def test_two_shards(form, oracle, paths):
    """Two shards, under each reduced-system form of a sharded plan
    (test_gpu_sharded.SOLVES; "whole", S all-reduced and solved by parallel
    cyclic reduction on every shard, is the default of this scene).  The
    solve rejects its first trial, so lmpar iterates: with S whole on every
    shard the Newton vector w has to be summed over the shards too
    (Plan::newton_enqueue) -- this scene found it taken from rank 0's rows
    alone (||f|| 5951.647627 at the third evaluation against the oracle's
    5984.737221; the unbounded scenes of the suite take the Gauss-Newton
    step every time and never got there)."""
    from tests.test_gpu_sharded import pin_solve
    pin_solve(paths, form)
    ctx = Context.multi([0, 0])
    try:
        def stats(s):
            assert s.num_shards == 2 and s.kernel_stats()["shards_replicated"] == 0
        run_case("c4_f40", oracle, ctx, stats=stats)
    finally:
        ctx.close()


@pytest.mark.parametrize("batch", [1, 0])
def test_per_frame(batch, oracle, paths):
    """Per-frame mode on the bounded C2 scene: the batch kernel's own
    reparametrisation and difference step (k_batch_lm), and with
    MMBA_PATH_PERFRAME_BATCH = 0 the sub-problem builder's gather of the four
    arrays; per frame against the oracle on sub-problems split here."""
    if not batch:
        paths(abi.PATH_PERFRAME_BATCH, 0)
    prob, opt = scene("c2_f6"), options("c2_f6")
    xr, rr = oracle_per_frame(prob, opt, oracle)
    assert len(rr) == prob.num_frames
    x, res = solve_per_frame(prob, opt, max_concurrency=4)
    check_frames(prob, res, rr, x, xr)
    frozen = S.bound_kinds(prob) == 1
    np.testing.assert_array_equal(prob.external_params(x)[frozen], prob.param_min[frozen])


# ---- c. the group back substitution ----

def solve_forms(case, ctx, paths):
    prob, opt = scene(SOLVES[case][0]), options(case)
    runs = {}
    for group, one in FORMS:
        paths(abi.PATH_BACKSUB_GROUP, group)
        paths(abi.PATH_BACKSUB_ONEPASS, one)
        s = Solver(prob, opt, context=ctx)
        try:
            runs[(group, one)] = s.solve()
        finally:
            s.close()
    ref = runs[FORMS[0]]
    assert ref.result["iterations"] > 2
    for k, r in runs.items():
        np.testing.assert_array_equal(r.x, ref.x, err_msg=str(k))
        np.testing.assert_array_equal(r.fnorm_trace, ref.fnorm_trace, err_msg=str(k))
        np.testing.assert_array_equal(r.fvec, ref.fvec, err_msg=str(k))
    # ... and form (0, 0) is the oracle's solve: not agreement in error
    check_whole_solve(case, ref)


@pytest.mark.parametrize("case", ["c4_f8-it8", "witness_g4-dag", "edge_parented"])
def test_group_forms_bit_identical(case, oracle, gpu_ctx, paths):
    """The four (GROUP, ONEPASS) forms of the trial back substitution on
    bounded scenes: the lane that owns a parameter loads its own xmin, xmax,
    offset and scale."""
    solve_forms(case, gpu_ctx, paths)


def test_group_forms_bit_identical_two_shards(oracle, paths):
    """The ownership mask of a sharded plan: each lane loads the bounds of
    the parameter it owns."""
    ctx = Context.multi([0, 0])
    try:
        solve_forms("c4_f40", ctx, paths)
    finally:
        ctx.close()


# ---- d. the fused large-plan path ----

@functools.lru_cache(maxsize=None)
def _fused_scene():
    prob = scene("c4_f257")
    return prob, S.config_options(prob, iterations=4)


def column_sample(prob, per_kind=24):
    """Columns of each kind -- differenced with a negative step, frozen,
    scaled, offset, and the rest -- spread over the parameter vector."""
    fl = S.flipped_columns(prob, 1e-4)
    frozen = S.bound_kinds(prob) == 1
    groups = [fl & ~frozen, frozen, prob.param_scale != 1.0, prob.param_offset != 0.0,
              ~fl & ~frozen]
    cols = set()
    for gsel in groups:
        idx = np.flatnonzero(gsel)
        assert idx.size >= per_kind
        cols.update(idx[np.linspace(0, idx.size - 1, per_kind).astype(int)].tolist())
    return np.array(sorted(cols))


def column_problem(prob, cols):
    """The problem with only ``cols`` solved and every other parameter written
    into the scene at its external value at x0: the oracle's Jacobian of it is
    those columns of the whole problem's (a column moves one parameter)."""
    d = prob.to_npz_dict()
    vals = np.array(d["attr_values"], dtype=np.float64)
    ext = prob.external_params(prob.x0)
    idx = prob.attr_offset[prob.param_attr] + np.where(
        prob.attr_animated[prob.param_attr] != 0, np.maximum(prob.param_frame, 0), 0)
    vals[idx] = ext
    d["attr_values"] = vals
    for k in ("param_attr", "param_frame", "param_min", "param_max", "param_offset",
              "param_scale", "x0"):
        d[k] = np.asarray(d[k])[cols]
    sub = type(prob).from_npz_dict(d)
    sub.meta = dict(prob.meta)
    return sub


def sparse_products(Jt, f, p, D, block=256):
    """From J^T (n x m, C order: one column of J per row) in numpy.longdouble,
    column block by column block over the rows each block touches: g = J^T f,
    the column norms, |J|^T |f| and J p."""
    n, m = Jt.shape
    g = np.zeros(n, np.longdouble)
    d2 = np.zeros(n, np.longdouble)
    ag = np.zeros(n)
    Jp = np.zeros(m, np.longdouble)
    fl, pl = f.astype(np.longdouble), p.astype(np.longdouble)
    for c0 in range(0, n, block):
        Jb = Jt[c0:c0 + block]
        rows = np.flatnonzero(np.any(Jb != 0., axis=0))
        if rows.size == 0:
            continue
        Jd = Jb[:, rows]
        Jl = Jd.astype(np.longdouble)
        g[c0:c0 + block] = Jl @ fl[rows]
        d2[c0:c0 + block] = np.sum(Jl * Jl, axis=1)
        ag[c0:c0 + block] = np.abs(Jd) @ np.abs(f[rows])
        Jp[rows] += Jl.T @ pl[c0:c0 + block]
    return g, d2, ag, Jp


def test_fused_first_iteration(oracle, gpu_ctx, paths):
    """257 camera-frames: the FD Jacobian and the camera-frame normal
    equations in one kernel (k_jac_ne_u), on bounded parameters.  One
    mmba_debug_damped_step call at lam = 1: g and D against the
    extended-precision J^T f and column norms of the call's own J
    (test_gpu_damped_step.py's bars), and the step p by its residual.  With
    B = D^-1 (J^T J + D^2) D^-1 and y = D p the system is B y = D^-1 g and
    B >= I, so ||y - y_exact||_2 <= ||B y - D^-1 g||_2: the residual, formed in
    extended precision, bounds the step's error, and is held to STEP_CAP
    (1e-7, the largest step bar test_gpu_damped_step.py admits) of ||y||_2.
    (Its dense reference costs a 9,033^2 factorisation here.)

    The same J twice more: a sample of its columns (negative step, frozen,
    scaled, offset, plain) against the oracle's Jacobian of column_problem,
    and all of it against the two-shard plan of the same scene, whose shards
    hold fewer than 256 camera-frames each and so run k_jacobian and the
    stand-alone normal equations (jac_ne_fusable)."""
    prob, opt = _fused_scene()
    n, m = prob.num_params, prob.num_residuals
    s = Solver(prob, opt, context=gpu_ctx)
    try:
        step, g, diag, J = s.damped_step(prob.x0, 1.0)
        f = s.measure(prob.x0)[0]
    finally:
        s.close()
    Jt = J.T  # C-contiguous (n, m)
    assert Jt.flags.c_contiguous
    assert np.all(np.isfinite(step)) and np.all(np.isfinite(g)) and np.all(np.isfinite(diag))
    frozen = S.bound_kinds(prob) == 1
    assert not np.any(Jt[frozen])
    D = np.sqrt(np.sum(Jt * Jt, axis=1))
    D[D == 0.] = 1.0
    g_ref, d2, abs_g, Jp = sparse_products(Jt, f, step, D)
    D_ref = np.sqrt(d2).astype(np.float64)
    D_ref[D_ref == 0.] = 1.0
    assert np.all(np.abs(g - g_ref.astype(np.float64)) <= 4.0 * m * EPS * abs_g)
    assert np.all(np.abs(diag - D_ref) <= 4.0 * m * EPS * D_ref)
    # the residual of the scaled system at the device's step
    JtJp = sparse_products(Jt, Jp.astype(np.float64), step, D)[0]  # J^T (J p), J p rounded once
    Dl = D_ref.astype(np.longdouble)
    r = (JtJp + Dl * Dl * step.astype(np.longdouble) - g_ref) / Dl
    y = D_ref * step
    res = float(np.linalg.norm(r.astype(np.float64)) / np.linalg.norm(y))
    print("fused c4_f257 n %d m %d  step residual %.2g of ||D p||" % (n, m, res))
    assert res <= STEP_CAP, res
    # a column sample against the oracle
    cols = column_sample(prob)
    sub = column_problem(prob, cols)
    f_ref, Js = oracle.jacobian(sub, opt, sub.x0)
    np.testing.assert_allclose(f, f_ref, rtol=1e-12, atol=1e-12)
    big = np.max(np.abs(Js))
    assert np.max(np.abs(Jt[cols].T - Js)) <= JAC_BAR * big
    fl = S.flipped_columns(sub, opt.delta) & (S.bound_kinds(sub) != 1)
    assert np.any(Js[:, fl] != 0.) and np.all(Jt[cols].T[:, fl][Js[:, fl] != 0.] != 0.)
    # the fused pass stood down: two shards
    bounds, _owner = shard_layout(prob, 2)
    cam_frames = [len(set(prob.obs_frame[(prob.obs_frame >= bounds[k]) &
                                         (prob.obs_frame < bounds[k + 1])].tolist()))
                  for k in range(2)]
    assert max(cam_frames) < 256 <= sum(cam_frames), cam_frames
    ctx = Context.multi([0, 0])
    try:
        s2 = Solver(prob, opt, context=ctx)
        try:
            assert s2.num_shards == 2
            step2, g2, diag2, J2 = s2.damped_step(prob.x0, 1.0)
        finally:
            s2.close()
    finally:
        ctx.close()
    J2t = J2.T
    worst = 0.0
    for c0 in range(0, n, 512):
        worst = max(worst, float(np.max(np.abs(J2t[c0:c0 + 512] - Jt[c0:c0 + 512]))))
    assert worst <= JAC_BAR * np.max(np.abs(Jt[cols])), worst
    assert np.all(np.abs(g2 - g) <= 8.0 * m * EPS * abs_g + JAC_BAR * big * np.sum(np.abs(f)))
    assert np.all(np.abs(diag2 - diag) <= 8.0 * m * EPS * D_ref + JAC_BAR * big * np.sqrt(m))


def test_fused_pass_and_fold_ran(gpu_ctx, paths):
    """The bounded 257-frame scene through the solve: the trial's reduction
    folded into the gated k_jac_ne_u launch behind it (trial_one_pre inside
    the fused trial writes the external values and difference steps that
    launch reads) against the stand-alone reduction, bit for bit, with the
    fold counted (mmba_kernel_stats.trial_red_folds) -- it is only ever taken
    behind the fused pass."""
    prob, opt = _fused_scene()
    runs = {}
    for fold in (0, 1):
        paths(abi.PATH_TRIAL_RED_FOLD, fold)
        s = Solver(prob, opt, context=gpu_ctx)
        try:
            r = s.solve()
            r.folds = s.kernel_stats()["trial_red_folds"]
            runs[fold] = r
        finally:
            s.close()
    assert runs[0].folds == 0
    assert runs[1].folds >= runs[1].result["outer_iterations"] - 1 > 0, runs[1].folds
    np.testing.assert_array_equal(runs[1].x, runs[0].x)
    np.testing.assert_array_equal(runs[1].fnorm_trace, runs[0].fnorm_trace)
    np.testing.assert_array_equal(runs[1].fvec, runs[0].fvec)
    frozen = S.bound_kinds(prob) == 1
    np.testing.assert_array_equal(prob.external_params(runs[1].x)[frozen],
                                  prob.param_min[frozen])
    assert np.all(np.isfinite(runs[1].fnorm_trace))
