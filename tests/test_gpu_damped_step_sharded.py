"""The damped LM step of sharded and group plans against the dense reference
of test_gpu_damped_step.py.

mmba_debug_damped_step on a sharded plan runs what a solve's first iteration
runs there -- fun, jac with the lmder bookkeeping, solve_damped_enqueue, with
the solve's collectives -- and hands back the step, g and D whole on every
rank (each parameter's entry from its owner) and the rows of J of the shard's
own observations.  The shards' J sum to the whole J; the reference is the
one of the unsharded test, built from that merged J and f (measure at x0):
it does not know about shards.  Bars, unchanged (m rows, eps = 2^-52):
  g     |g - g_ref| <= 4 m eps (|J|^T |f|)  componentwise
  D     |D - D_ref| <= 4 m eps D_ref
  step  max|D (p - p_ref)| / max|D p_ref| <= 1000 e64 of the merged device J;
        a (scene, lam) pair is admissible only if 1000 e64 <= 1e-7 on the
        oracle's J (test_one_observation_moves_the_reference, CPU).
Per case, besides the bars: every observation's rows are non-zero in exactly
one shard's J; the merged J is the unsharded plan's hook J within 1e-7 of its
largest entry; every threaded shard returns the same bits; the group plan
(Context.multi) returns the threaded shards' bits; the statistics say the
pinned reduced-solve form ran; and zeroing one observation at a seam (an own
observation in a shard's last frame, one in the next shard's first frame, a
halo observation -- ownership from mmba_shard_layout, checked against the
shards' rows) moves the reference step by at least 1000 x the step bar.

Scenes: the smallest that still shard (shards_replicated == 0 asserted).
Plan::build needs 2 bw + 8 camera-frame rows on every shard: 54 rows (9
frames) at the C4 spec's 4-frame tracks (bw 23), 78 rows (13 frames) at
6-frame tracks (bw 35); the partition follows the observation count, so its
smallest shard decides (frames per shard in SCENES, from mmba_shard_layout).
The separator form needs bw <= 23 and no arrow: on the 6-frame scenes its pin
stands down by design (Plan::sep_form) and so does the log-depth whole-S
solve (bw <= 32), so the three pins build the same plan there -- the band
chains with an all-reduced separator system, band_solver 1 -- which the
statistics must say.  A sharded C2 plan holds its block-diagonal system as
a band of bw 6 (the one-launch block-diagonal solver is unsharded only), so
the three forms apply to it.  C3 shards at test size (shard_dense).

Left out: shards of >= 256 camera-frames (k_jac_ne_u).  Two of them are 512
camera-frames x 6 parameters, and the library refuses m < n ("more parameters
than errors"), so the smallest such scene has n = 4,491 (560 frames, 380
six-frame bundles; 291 and 269 frames per shard).  The reference costs 7.9 s
at n = 3,351 on the CPU (cubic: about 20 s there) and the seam mutations
need three more: not a test of seconds.  test_gpu_group.py::
test_group_fused_jacobian_shards keeps that path at its whole-solve bar.

Pairs left out (lam = 0 only), in LEFT_OUT with their e64 on the oracle's J.

B15 plans (lmder with central differences over animated parameters of several
frames) are unsharded by Plan::build; their step is held to the same bars in
test_gpu_damped_step_b15.py.

Measured on an MI355X, e64 / the device's error (the step measure, on the
merged device J; g and D stayed below 2e-4 of their bars everywhere; the ring
order gave the same figures to two digits; every run prints these lines with
-s; profiles/r10_step_sharded/):

scene       form            n      m  lam 1              lam 1e-3           lam 0
c4_n2       separator     831   1600  4.7e-15 / 1.1e-15  2.1e-13 / 3.1e-14  left out
c4_n2       whole         831   1600  4.7e-15 / 8.6e-16  2.1e-13 / 3.9e-14  left out
c4_n2       partitioned   831   1600  4.7e-15 / 8.1e-16  2.1e-13 / 4.6e-14  left out
c4_n3       separator    1251   2400  2.8e-15 / 9.4e-16  4e-13 / 3.7e-14    left out
c4_n3       whole        1251   2400  2.8e-15 / 9.3e-16  4e-13 / 6.3e-14    left out
c4_n3       partitioned  1251   2400  2.8e-15 / 6.4e-16  4e-13 / 4.6e-14    left out
c4_n4       separator    1335   2560  1.3e-14 / 8.4e-16  5e-13 / 4.8e-14    left out
c4_n4       whole        1335   2560  1.3e-14 / 1.1e-15  5e-13 / 8.4e-14    left out
c4_n4       partitioned  1335   2560  1.3e-14 / 8e-16    5e-13 / 5.1e-14    left out
c4_n8       separator    1503   2240  1.7e-14 / 1.2e-15  2e-13 / 1e-13      left out
c4_n8       whole        1503   2240  1.7e-14 / 7.5e-16  2e-13 / 1.6e-13    left out
c4_n8       partitioned  1503   2240  1.7e-14 / 8.6e-16  2e-13 / 4.3e-14    left out
wc_n2       separator     831   2400  5.3e-15 / 9.3e-16  1.3e-13 / 5.7e-14  2.3e-12 / 4.8e-13
wc_n2       whole         831   2400  5.3e-15 / 9.3e-16  1.3e-13 / 5.7e-14  2.3e-12 / 4.8e-13
wc_n2       partitioned   831   2400  5.3e-15 / 9.3e-16  1.3e-13 / 5.7e-14  2.3e-12 / 4.8e-13
wc_n4       separator    1503   4320  1.5e-15 / 8.8e-16  1.9e-13 / 3.7e-14  3.8e-11 / 3.1e-12
wc_n4       whole        1503   4320  1.5e-15 / 8.8e-16  1.9e-13 / 3.7e-14  3.8e-11 / 3.1e-12
wc_n4       partitioned  1503   4320  1.5e-15 / 8.8e-16  1.9e-13 / 3.7e-14  3.8e-11 / 3.1e-12
c2_n2       separator     168  11904  1.2e-15 / 4e-16    3.1e-15 / 1.5e-15  3.3e-15 / 1.2e-15
c2_n2       whole         168  11904  1.2e-15 / 5.6e-16  3.1e-15 / 1.5e-15  3.3e-15 / 9.3e-16
c2_n2       partitioned   168  11904  1.2e-15 / 5.4e-16  3.1e-15 / 9.4e-16  3.3e-15 / 1.6e-15
c2_n3       separator     252  16476  1.3e-15 / 3.4e-16  3.2e-15 / 9.7e-16  3.4e-15 / 1.2e-15
c2_n3       whole         252  16476  1.3e-15 / 4e-16    3.2e-15 / 9.6e-16  3.4e-15 / 1.2e-15
c2_n3       partitioned   252  16476  1.3e-15 / 3.8e-16  3.2e-15 / 9.3e-16  3.4e-15 / 6.5e-16
c5_n2       whole         386   6400  1.8e-15 / 6.9e-16  2.1e-14 / 1.2e-15  2.2e-14 / 1.5e-15
c5_n2       partitioned   386   6400  1.8e-15 / 1.4e-15  2.1e-14 / 4.7e-15  2.2e-14 / 1.2e-15
c5_anim_n2  whole         225   6400  1.3e-15 / 6.4e-16  4.1e-15 / 1.2e-15  3.8e-15 / 1.7e-15
c3_n2       whole         531   1600  1.8e-15 / 9.3e-16  5.2e-14 / 4.8e-14  1.8e-12 / 2.6e-12

The largest device error is 1.4 x e64 (c3_n2 at lam = 0), against the margin
of 1000.  With the halo left out of the bundles' g (scratch build) g stands
3.6e11 x above its bar and the step error is 0.23 against a bar of 2.8e-12
(c4_n3); with a step row gathered from the wrong rank the step error is 1.4
to 1.7 on every plan that gathers rows (the separator form and the band
chains; the log-depth whole-S solve gathers none).
"""
import functools

import numpy as np
import pytest

from mayamatchmovesolver_amd import abi, synthetic as S
from mayamatchmovesolver_amd.solver import Context, Solver, shard_layout

# (the step bar is Reference.step_bar: STEP_MARGIN x e64, as in the unsharded test)
from test_gpu_damped_step import (BAND, DENSE, EPS, LAMS, STEP_CAP, STEP_CAP_DEVICE, Reference,
                                  step_error)
from test_gpu_sharded import ORDERS, SOLVES, run_sharded

gpu = pytest.mark.gpu

WC = dict(window=6, depth=(4.0, 10.0))
COMM_TIMEOUT_MS = 30000  # a shard that fails ends the test, not the 120 s default
JAC_BAR = 1e-7           # the project's Jacobian bar, of the largest entry


def _cfg(index, **kw):
    return lambda: S.make_config(index, **kw)


# name: factory, shard count, the reduced-solve forms and summation orders run,
# reduced_kind, band_solver per form, whether bundles are solved (a halo exists)
def _s(make, n, forms, orders, kind, solver, halo, lams=LAMS):
    return dict(make=make, n=n, forms=forms, orders=orders, kind=kind, solver=solver, halo=halo,
                lams=list(lams))


ALL = list(SOLVES)
BOTH = list(ORDERS)
# band_solver (mmba_kernel_stats): 1 band Cholesky / partitioned chains, 2
# block cyclic reduction, 3 parallel cyclic reduction, 4 the separator form,
# 5 block diagonal
C4_SOLVER = {"separator": (4,), "whole": (2, 3), "partitioned": (1,)}
# bw 35: no separator form, no log-depth solver -- the band chains whatever is pinned
WC_SOLVER = {"separator": (1,), "whole": (1,), "partitioned": (1,)}
SCENES = {
    # ---- C4 spec, 4-frame tracks (bw 23); frames per shard as partitioned ----
    "c4_n2": _s(_cfg(3, frames=40, scale=0.004), 2, ALL, BOTH, BAND, C4_SOLVER, True),
    # a middle shard: separators on both sides
    "c4_n3": _s(_cfg(3, frames=60, scale=0.006), 3, ALL, BOTH, BAND, C4_SOLVER, True),
    # 17, 17, 12, 18 frames
    "c4_n4": _s(_cfg(3, frames=64, scale=0.0064), 4, ALL, BOTH, BAND, C4_SOLVER, True),
    # the deepest separator system; 17, 12, 16, 14, 10, 12, 15, 16 frames
    "c4_n8": _s(_cfg(3, frames=112, scale=0.0056), 8, ALL, BOTH, BAND, C4_SOLVER, True),
    # ---- 6-frame tracks (bw 35): the band the partitioned form takes ----
    "wc_n2": _s(_cfg(3, frames=40, scale=0.004, **WC), 2, ALL, BOTH, BAND, WC_SOLVER, True),
    # 19, 19, 14, 20 frames
    "wc_n4": _s(_cfg(3, frames=72, scale=0.0072, **WC), 4, ALL, BOTH, BAND, WC_SOLVER, True),
    # ---- C2: no Schur complement; block diagonal, which a sharded plan holds
    # as a band of bw 6 (the one-launch block-diagonal solver is unsharded
    # only, Plan::build), so the three forms apply ----
    "c2_n2": _s(_cfg(1, frames=24, scale=0.05), 2, ALL, ["rank"], BAND, C4_SOLVER, False),
    "c2_n3": _s(_cfg(1, frames=36, scale=0.05), 3, ALL, ["rank"], BAND, C4_SOLVER, False),
    # ---- C5: lens globals, the arrow rows, the d_Agg all-reduce; with an
    # arrow there is no separator form and no parallel cyclic reduction ----
    "c5_n2": _s(_cfg(4, frames=32, scale=0.05), 2, ["whole", "partitioned"], BOTH, BAND,
                {"whole": (2,), "partitioned": (1,)}, False),
    # the distortion keyed per frame (in the camera-frame block), the quartic
    # coefficient global
    "c5_anim_n2": _s(_cfg(4, frames=32, scale=0.05, lens_model="classic_animated", cameras=1), 2,
                     ["whole"], ["rank"], BAND, {"whole": (2,)}, False),
    # ---- C3 class: the shards' dense S all-reduced (shard_dense) ----
    "c3_n2": _s(_cfg(2, frames=8, scale=0.002), 2, ["whole"], ["rank"], DENSE, {"whole": None},
                True),
}

# (scene, lam): e64 on the oracle's J -- 1000 e64 above STEP_CAP, no sharp bar
LEFT_OUT = {
    # the C4 spec's far bundles on a short baseline: the undamped normal
    # equations are too ill-conditioned for a sharp fp64 bar
    ("c4_n2", 0.0): 4.4e-10,
    ("c4_n3", 0.0): 5.4e-10,
    ("c4_n4", 0.0): 1.6e-9,
    # ten observations per frame: frames with too few for six parameters,
    # J^T J is singular without damping
    ("c4_n8", 0.0): 1.0,
}
# scenes whose FD Jacobian is too slow for the oracle on the CPU: admissibility
# and power on the device's J instead (test_sharded_damped_step); none today
SLOW_ON_CPU = set()


def lams_of(name):
    return [lam for lam in SCENES[name]["lams"] if (name, lam) not in LEFT_OUT]


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name]["make"]()


def options(name):
    return S.config_options(scene(name))


# ---- seams ----

def obs_bundle(prob):
    return np.asarray(prob.mkr_bnd)[np.asarray(prob.obs_marker)]


def seam_observations(prob, bounds, live, k, halo):
    """Observations at the seam between shards k and k + 1 (frames
    [bounds[k], bounds[k + 1]) and the next range): an own observation of
    shard k nearest its last frame, one of shard k + 1 nearest its first
    frame, and (halo) an observation shard k holds for a bundle its frames
    see although the observation's frame is another shard's."""
    fr = np.asarray(prob.obs_frame)
    a, b, c = int(bounds[k]), int(bounds[k + 1]), int(bounds[k + 2])
    mine = np.flatnonzero(live & (fr >= a) & (fr < b))
    nxt = np.flatnonzero(live & (fr >= b) & (fr < c))
    out = {"last frame": int(mine[np.argmax(fr[mine])]),
           "next shard's first frame": int(nxt[np.argmin(fr[nxt])])}
    if halo:
        bnd = obs_bundle(prob)
        seen = np.zeros(prob.num_bundles, bool)
        seen[bnd[(fr >= a) & (fr < b)]] = True
        h = np.flatnonzero(live & seen[bnd] & ~((fr >= a) & (fr < b)))
        assert h.size, "no halo observation at seam %d" % k
        h = h[h != out["next shard's first frame"]]
        out["halo"] = int(h[np.argmax(fr[h])])  # the one farthest into the next shard
    return out


def check_seams(name, J, f, ref, bounds, lams):
    """Zeroing the two rows of one seam observation moves the reference step
    by at least 1000 x the step bar (check_power's threshold), at the first
    seam and, with a middle shard, at the last."""
    sc, prob = SCENES[name], scene(name)
    M = prob.num_obs
    live = np.any(J[:2 * M].reshape(M, 2, -1) != 0., axis=(1, 2))
    seams = sorted({0, sc["n"] - 2})
    D = ref.D.astype(np.float64)
    for k in seams:
        for what, i in seam_observations(prob, bounds, live, k, sc["halo"]).items():
            Jz = J.copy()
            Jz[2 * i:2 * i + 2] = 0.
            rz = Reference(Jz, f)
            for lam in lams:
                moved = step_error(rz.step(lam)[0], ref.step(lam)[0], D)
                print("%-12s seam %d lam %-6g %-26s obs %5d moves the step by %.2g (bar %.2g)"
                      % (name, k, lam, what, i, moved, ref.step_bar(lam)))
                assert moved >= 1000.0 * ref.step_bar(lam), (name, k, what, lam, moved)


# ---- CPU: admissibility and power, on the oracle's J ----

@functools.lru_cache(maxsize=None)
def oracle_reference(name):
    from oracle import refcpu
    prob = scene(name)
    f, J = refcpu.jacobian(prob, options(name), prob.x0)
    J = np.ascontiguousarray(J)
    return Reference(J, f), J, f


CPU_SCENES = sorted(n for n in SCENES if n not in SLOW_ON_CPU)


@pytest.mark.parametrize("name", CPU_SCENES)
def test_one_observation_moves_the_reference(name):
    """Every (scene, lam) pair tested is admissible (1000 e64 <= 1e-7 on the
    oracle's J) and a seam observation moves the reference step by at least
    1000 x the step bar."""
    ref, J, f = oracle_reference(name)
    lams = lams_of(name)
    for lam in SCENES[name]["lams"]:
        print("%-12s lam %-6g n %4d e64 %.2g%s" % (name, lam, J.shape[1], ref.step(lam)[1],
                                                 "" if lam in lams else "  left out"))
    for lam in lams:
        assert ref.step_bar(lam) <= STEP_CAP, (lam, ref.step(lam)[1])
    check_seams(name, J, f, ref, shard_layout(scene(name), SCENES[name]["n"])[0], lams)


def test_left_out_pairs():
    """Only lam = 0 is ever left out, and only where the plain fp64
    evaluation has no sharp bar (1000 e64 > 1e-7 on the oracle's J)."""
    for (name, lam), e in LEFT_OUT.items():
        assert lam == 0.0 and name in SCENES and name not in SLOW_ON_CPU
        ref, _J, _f = oracle_reference(name)
        assert ref.step_bar(lam) > STEP_CAP, (name, ref.step(lam)[1])


# ---- GPU ----

_runs, _refs, _single = {}, {}, {}


def pin(paths, form, order):
    for k, v in SOLVES[form].items():
        paths(k, v)
    paths(abi.PATH_LOCAL_RING, ORDERS[order])
    paths(abi.PATH_COMM_TIMEOUT_MS, COMM_TIMEOUT_MS)


def hook_all_lams(name):
    prob = scene(name)

    def call(s):
        out = {lam: s.damped_step(prob.x0, lam) for lam in lams_of(name)}
        return out, s.measure(prob.x0)[0]
    return call


def threaded_run(name, form, order, paths):
    """One sharded plan per (scene, form, order), on one host thread per
    shard: every lam's hook outputs and f of every shard, and the statistics."""
    key = (name, form, order)
    if key not in _runs:
        pin(paths, form, order)
        sc = SCENES[name]
        stats = []
        outs = run_sharded(scene(name), options(name), sc["n"], stats=stats,
                           call=hook_all_lams(name))
        _runs[key] = (outs, stats)
    return _runs[key]


def group_run(name, form, order, paths):
    pin(paths, form, order)
    n = SCENES[name]["n"]
    ctx = Context.multi([0] * n)
    try:
        s = Solver(scene(name), options(name), context=ctx)
        try:
            assert s.num_shards == n
            return hook_all_lams(name)(s)
        finally:
            s.close()
    finally:
        ctx.close()


def single_J(name, ctx):
    """The unsharded plan's hook J at x0."""
    if name not in _single:
        prob = scene(name)
        s = Solver(prob, options(name), context=ctx)
        try:
            _single[name] = s.damped_step(prob.x0, 1.0)[3]
        finally:
            s.close()
    return _single[name]


def merged(name, outs, lam0):
    """The shards' J summed; every observation's two rows non-zero in at most
    one shard's (and every live one in exactly one)."""
    M = scene(name).num_obs
    Js = [o[0][lam0][3] for o in outs]
    holds = np.stack([np.any(J[:2 * M].reshape(M, 2, -1) != 0., axis=(1, 2)) for J in Js])
    assert holds.sum(axis=0).max() <= 1, "an observation's rows in two shards"
    J = Js[0].copy()
    for Jk in Js[1:]:
        J += Jk
    return np.ascontiguousarray(J), holds


def reference_of(name, J, f):
    """One reference per scene: the Jacobian pass does not depend on the
    reduced-solve form or the summation order, so J repeats bit for bit."""
    if name in _refs and np.array_equal(_refs[name][0], J) and np.array_equal(_refs[name][1], f):
        return _refs[name][2]
    ref = Reference(J, f)
    _refs[name] = (J, f, ref)
    return ref


def check_bars(name, what, lam, out, ref):
    step, g, diag = out[:3]
    p_ref, e64 = ref.step(lam)
    D = ref.D.astype(np.float64)
    m = ref.m
    g_ref = ref.g.astype(np.float64)
    g_bar = 4.0 * m * EPS * ref.abs_g
    g_err = float(np.max(np.abs(g - g_ref) / np.maximum(g_bar, np.finfo(float).tiny)))
    d_err = float(np.max(np.abs(diag - D) / (4.0 * m * EPS * D)))
    err = step_error(step, p_ref, D)
    print("%-12s %-22s lam %-6g n %4d m %6d  e64 %.2g  bar %.2g  device %.2g  (g %.2g, D %.2g "
          "of their bars)" % (name, what, lam, D.size, m, e64, ref.step_bar(lam), err, g_err,
                              d_err))
    assert np.all(np.isfinite(step)) and np.all(np.isfinite(g)) and np.all(np.isfinite(diag))
    assert ref.step_bar(lam) <= STEP_CAP_DEVICE, "no sharp bar on this J: e64 %.3g" % e64
    assert np.all(np.abs(g - g_ref) <= g_bar), "g: %.3g of its bar" % g_err
    assert np.all(np.abs(diag - D) <= 4.0 * m * EPS * D), "D: %.3g of its bar" % d_err
    assert err <= ref.step_bar(lam), "step: %.3g against %.3g" % (err, ref.step_bar(lam))


CASES = [pytest.param(name, form, order, id="%s-%s-%s" % (name, form, order))
         for name, sc in SCENES.items() for form in sc["forms"] for order in sc["orders"]]


@gpu
@pytest.mark.parametrize("name,form,order", CASES)
def test_sharded_damped_step(name, form, order, gpu_ctx, paths):
    """The hook on threaded shards and on the group plan, at every admissible
    lam, against the reference of the merged device J (module docstring)."""
    sc, prob = SCENES[name], scene(name)
    n, lams = sc["n"], lams_of(name)
    outs, stats = threaded_run(name, form, order, paths)
    # really sharded, on the pinned form
    assert [st["shards_replicated"] for st in stats] == [0] * n
    for st in stats:
        assert st["reduced_kind"] == sc["kind"], st
        if sc["solver"][form] is not None:
            assert st["band_solver"] in sc["solver"][form], (form, st["band_solver"])
    # the same pass at the same x: the same J at every lam; f the same on every shard
    for o in outs:
        for lam in lams[1:]:
            np.testing.assert_array_equal(o[0][lam][3], o[0][lams[0]][3])
        np.testing.assert_array_equal(o[1], outs[0][1])
    f = outs[0][1]
    J, holds = merged(name, outs, lams[0])
    bounds, _owner = shard_layout(prob, n)
    fr = np.asarray(prob.obs_frame)
    for k in range(n):  # rows only of the shard's own frames
        assert not np.any(holds[k] & ~((fr >= bounds[k]) & (fr < bounds[k + 1]))), k
    # the merged J is the unsharded plan's
    J1 = single_J(name, gpu_ctx)
    assert np.max(np.abs(J - J1)) <= JAC_BAR * np.max(np.abs(J1))
    np.testing.assert_array_equal(holds.any(axis=0),
                                  np.any(J1[:2 * prob.num_obs].reshape(prob.num_obs, 2, -1) != 0.,
                                         axis=(1, 2)))
    ref = reference_of(name, J, f)
    what = "%s/%s" % (form, order)
    for lam in lams:
        check_bars(name, what, lam, outs[0][0][lam], ref)
        for o in outs[1:]:  # every shard: the same bits
            for a, b, w in zip(o[0][lam][:3], outs[0][0][lam][:3], ("step", "g", "D")):
                np.testing.assert_array_equal(a, b, err_msg="%s at lam %g" % (w, lam))
    # the group plan: the threaded shards' bits, and the merged J in one array
    gout, gf = group_run(name, form, order, paths)
    np.testing.assert_array_equal(gf, f)
    for lam in lams:
        for a, b, w in zip(gout[lam][:3], outs[0][0][lam][:3], ("step", "g", "D")):
            np.testing.assert_array_equal(a, b, err_msg="group %s at lam %g" % (w, lam))
        np.testing.assert_array_equal(gout[lam][3], J)
    if (form, order) == (sc["forms"][0], sc["orders"][0]):
        if name in SLOW_ON_CPU:
            for lam in lams:
                assert ref.step_bar(lam) <= STEP_CAP, (lam, ref.step(lam)[1])
        check_seams(name, J, f, ref, bounds, lams)


@gpu
def test_hook_refusals_and_repeats(paths):
    """On a sharded plan a second call repeats the first bit for bit, and so
    does a call after a solve()."""
    name = "c4_n2"
    prob = scene(name)
    pin(paths, "whole", "rank")

    def call(s):
        a = s.damped_step(prob.x0, 1e-3)
        b = s.damped_step(prob.x0, 1e-3)
        s.solve()
        c = s.damped_step(prob.x0, 1e-3)
        return a, b, c
    for a, b, c in run_sharded(prob, S.config_options(prob, iterations=3), 2, call=call):
        for u, v, w in zip(a, b, c):
            np.testing.assert_array_equal(u, v)
            np.testing.assert_array_equal(u, w)
