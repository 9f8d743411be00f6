"""The damped LM step of every assembly path against a dense reference.

Between the FD Jacobian and the trial point one LM iteration runs the normal
equations (k_ne_cf*, k_jac_ne_u, k_ne_bnd*, k_ne_glob*), the Schur complement
(k_bundle_factor, k_schur_*), a reduced solver and the back substitution.
Which variant runs depends on the scene's shape.  mmba_debug_damped_step runs
that chain once at x0 as a solve's first iteration does and hands back the
step p, g, D and the dense J the pass stored; with MINPACK's first-call
scaling D = diag(||J col||) (1 for a zero column) p must solve

    (J^T J + lam D^2) p = SIGN J^T f,   SIGN = +1

(Plan::solve_damped_enqueue: d_xs = (A + lam D^2)^-1 g; the trial point is
x - xs).  J and f are the device's own, so FD rounding and the Jacobian's own
1e-7 bar stay out of the comparison.  The reference forms A = J^T J and
g = J^T f in numpy.longdouble and solves in fp64 with four steps of iterative
refinement against the extended-precision residual.

Bars, from the reference alone (m = rows of J, eps = 2^-52):
  g     |g - g_ref|    <= 4 m eps (|J|^T |f|)   componentwise
  D     |D - D_ref|    <= 4 m eps D_ref
  step  max|D (p - p_ref)| / max|D p_ref| <= 1000 e64, where e64 is the same
        measure of the plain fp64 numpy evaluation of the formula on the same
        J and f; a (scene, lam) pair is admissible only if 1000 e64 <= 1e-7
        (on the oracle's J, test_one_observation_moves_the_reference).
With that scaling the damped matrix has unit diagonal plus lam, so at
lam = 1 its condition number is at most n + 1 on any scene.
test_one_observation_moves_the_reference (CPU, the oracle's J) holds every
scene to "zeroing one observation's two rows moves the reference step by at
least 1000 x the step bar": a scene too flat to notice a dropped observation
cannot pass silently.

Pairs left out (lam = 0 only), by name, in LEFT_OUT with their e64.

Sharded and group plans: test_gpu_damped_step_sharded.py, the same reference
and bars.

B15 plans (central differences: with lmder every scene whose animated
parameters span several frames builds a B15 plan or none, Plan::build; lmdif
has forward differences only): test_gpu_damped_step_b15.py, the same bars
against a yardstick in the plan's rotated basis.

Not reached: k_schur_pairs (Plan::build takes it only above 2^30 destination
pairs);
  per-frame batch plans: mmba_plan_solve_per_frame runs its own batched LM
    (mmba_batch.hip), which has no single damped step to hand back.

Measured on an MI355X, e64 / the device's error (the step measure, on the
device's J; g and D stayed below 1.1e-3 of their bars everywhere; every run
prints these lines with -s):

scene               n      m  lam 1              lam 1e-3           lam 0
c4_f8             189    400  1.8e-15 / 6.2e-16  1.7e-13 / 3.2e-14  7.8e-11 / 1.5e-11
c4_f8_pcr         189    400  1.8e-15 / 6.2e-16  1.7e-13 / 3.2e-14  7.8e-11 / 1.5e-11
c4_f8_bcr         189    400  1.8e-15 / 6.8e-16  1.7e-13 / 3.2e-14  7.8e-11 / 1.7e-11
c4_f64            975   2400  3.8e-15 / 1.3e-15  1.2e-13 / 5.0e-14  2.6e-11 / 1.3e-11
c4_f32_pcr        783   1600  2.3e-15 / 7.3e-16  1.5e-13 / 6.9e-14  1.8e-11 / 5.6e-12
c4_f40_bcr        831   2000  2.3e-15 / 1.4e-15  9.6e-14 / 5.7e-14  2.8e-12 / 1.3e-12
c4_f257          2283   3000  1.6e-14 / 1.2e-15  2.1e-12 / 1.2e-13  left out (singular)
c2_pc7             84   6000  6.9e-16 / 4.0e-16  1.7e-15 / 8.6e-16  1.2e-15 / 6.1e-16
c2_pc6             72   6000  6.9e-16 / 4.2e-16  1.5e-15 / 6.6e-16  1.2e-15 / 7.0e-16
c5_f8              98   1600  1.0e-15 / 5.9e-16  3.2e-15 / 9.5e-16  2.1e-15 / 9.2e-16
c5_f4_wide         50   3200  1.6e-15 / 3.8e-16  8.9e-15 / 1.7e-15  8.1e-15 / 1.1e-15
c5_pc7            114   1600  1.2e-15 / 6.6e-16  1.8e-14 / 8.4e-15  1.7e-14 / 7.9e-15
c5_pc7_wide        58   3200  1.3e-15 / 3.6e-16  3.9e-15 / 8.7e-15  4.1e-15 / 8.6e-15
c5_65chunks        14  65600  7.9e-16 / 1.9e-16  2.2e-15 / 4.2e-15  1.6e-15 / 1.7e-15
c5_wide12          72   1200  1.0e-15 / 9.2e-16  2.2e-15 / 1.8e-15  left out (singular)
wit_g4            112    864  9.2e-16 / 5.5e-16  5.1e-14 / 1.6e-14  2.3e-13 / 6.5e-14
wit_g5            113    864  9.3e-16 / 7.4e-16  9.9e-15 / 1.5e-14  4.2e-14 / 6.6e-14
wit_g11           119   1152  7.4e-16 / 7.8e-16  5.3e-14 / 1.6e-14  5.3e-14 / 4.2e-14
wit_g16           112    960  7.4e-16 / 1.2e-15  8.1e-14 / 3.0e-14  1.9e-13 / 1.3e-14
wit_g40           136   1536  1.8e-15 / 2.0e-15  1.4e-13 / 9.2e-14  8.4e-13 / 5.7e-13
wit_lens_g14      122    864  1.5e-15 / 6.6e-16  6.5e-14 / 1.0e-13  1.4e-11 / 9.4e-12
wit_wide_block    148    864  2.0e-14 / 1.0e-15  4.0e-14 / 7.3e-14  left out (singular)
wit_bd_g4          40    864  3.8e-16 / 5.7e-16  4.5e-15 / 5.3e-15  5.2e-15 / 4.7e-15
wit_bd_g11         47   1152  3.3e-15 / 5.6e-16  2.7e-14 / 1.4e-14  3.0e-14 / 1.3e-14
wit_bd_g16         40    960  8.9e-16 / 9.2e-16  2.1e-14 / 6.0e-15  2.2e-14 / 4.0e-15
c3_tiled_lane0    291    800  1.9e-15 / 1.1e-15  6.8e-14 / 2.4e-14  1.4e-12 / 4.5e-12
c3_tiled_lane1    291    800  1.9e-15 / 1.1e-15  6.8e-14 / 2.4e-14  1.4e-12 / 4.5e-12
c3_dense          291    800  1.9e-15 / 8.2e-16  6.8e-14 / 2.0e-14  1.4e-12 / 7.8e-14
edge_dup           99    324  8.2e-16 / 8.9e-16  4.9e-14 / 2.4e-14  1.3e-12 / 1.1e-13
edge_g1           100    288  6.8e-16 / 4.2e-16  1.8e-13 / 8.0e-14  3.2e-13 / 6.6e-13
edge_g3           102    288  1.4e-15 / 1.1e-15  5.2e-14 / 4.5e-14  left out (e64 17)
edge_rows          99    291  5.9e-16 / 4.1e-16  1.3e-13 / 1.5e-14  8.7e-13 / 1.6e-12
edge_rs            99    288  1.2e-15 / 8.8e-16  5.1e-14 / 2.1e-14  6.5e-13 / 1.3e-12

The largest device error is 3.2 x e64 (c3_tiled at lam = 0), against the
margin of 1000.
"""
import functools

import numpy as np
import pytest

from mayamatchmovesolver_amd import abi, make_options, synthetic as S
from mayamatchmovesolver_amd.solver import Solver

gpu = pytest.mark.gpu

SIGN = 1.0
LAMS = [1.0, 1e-3, 0.0]
EPS = 2.0 ** -52
STEP_MARGIN = 1000.0   # x e64: another summation order and the two-stage elimination
STEP_CAP = 1e-7        # 1000 e64 above this: the pair is not admissible
# Admissibility is a property of the scene, decided where it was measured: on
# the oracle's J (CPU).  e64 is the rounding error of one ill-conditioned fp64
# solve, so on the device's J (other roundings of the same entries) it moves
# by a small factor; the bar stays 1000 e64 of the J at hand, and a bar more
# than ten times the cap fails the case: the one-observation mutation, held
# to 1000 x the bar on the CPU, then still stands 100 x above it.
STEP_CAP_DEVICE = 10.0 * STEP_CAP
MMSG, DAG = abi.SCENE_GRAPH_MODE_MM_SCENE_GRAPH, abi.SCENE_GRAPH_MODE_MAYA_DAG
# mmba_kernel_stats: reduced_kind / band_solver
BAND, TILED, DENSE, BDIAG = 0, 1, 2, 3
S_NONE, S_CHOL, S_BCR, S_PCR, S_PCRI, S_BD = 0, 1, 2, 3, 4, 5


def _rs_parented():
    p = S.edge_scene(parented=True, solve_bundles=True)
    p.cam_rs_value = np.array([0.6])
    return p


def _cfg(index, **kw):
    return lambda: S.make_config(index, **kw)


def _wit(**kw):
    return lambda: S.witness_scene(**kw)


def _edge(**kw):
    return lambda: S.edge_scene(**kw)


# name: factory, options ("config": synthetic.config_options, else make_options),
# scene-graph mode, path pins, and the structural facts the dispatch rests on:
# M observations, cf camera-frames with observations, nG globals, pcs = the
# distinct per-frame solved parameter counts, kind / solver from kernel_stats.
# "reaches": the kernels the scene is here for (read off launch_ne,
# launch_schur_dest and Plan::solve_damped_enqueue).
def _s(make, reaches, M, cf, nG, pcs, kind, solver, opt="config", mode=MMSG, pins=None,
       same_as=None):
    return dict(make=make, reaches=reaches, M=M, cf=cf, nG=nG, pcs=pcs, kind=kind,
                solver=solver, opt=opt, mode=mode, pins=pins or {}, same_as=same_as)


SCENES = {
    # ---- no globals, solved bundles (C4 class) ----
    "c4_f8": _s(_cfg(3, frames=8, scale=0.001),
                "k_ne_cf_u<6,1,0>, k_ne_bnd_jb, k_schur_init folded into k_schur_dest_u<6>",
                200, 8, 0, [6], BAND, (S_PCR, S_PCRI)),
    "c4_f8_pcr": _s(_cfg(3, frames=8, scale=0.001), "parallel cyclic reduction",
                    200, 8, 0, [6], BAND, (S_PCR, S_PCRI), pins={abi.PATH_PCR: 1}, same_as="c4_f8"),
    "c4_f8_bcr": _s(_cfg(3, frames=8, scale=0.001), "block cyclic reduction",
                    200, 8, 0, [6], BAND, (S_BCR,), pins={abi.PATH_PCR: 0}, same_as="c4_f8"),
    # half bandwidth 35: the band Cholesky
    "c4_f64": _s(_cfg(3, frames=64, scale=0.004, window=6, depth=(4, 10)),
                 "band Cholesky without an arrow over 64 blocks", 1200, 64, 0, [6], BAND,
                 (S_CHOL,)),
    # half bandwidth 23 (K = 24): parallel cyclic reduction over 32 blocks
    "c4_f32_pcr": _s(_cfg(3, frames=32, scale=0.004, window=4, depth=(4, 10)),
                     "parallel cyclic reduction, five levels", 800, 32, 0, [6], BAND,
                     (S_PCR, S_PCRI), pins={abi.PATH_PCR: 1}),
    # half bandwidth 29 (K = 32): block cyclic reduction over 40 blocks
    "c4_f40_bcr": _s(_cfg(3, frames=40, scale=0.004, window=5, depth=(4, 10)),
                     "block cyclic reduction, K = 32", 1000, 40, 0, [6], BAND,
                     (S_BCR,), pins={abi.PATH_PCR: 0}),
    # >= 256 camera-frames: the Jacobian and the camera-frame normal equations
    # in one kernel
    "c4_f257": _s(_cfg(3, frames=257, scale=0.005, window=6, depth=(4, 10)),
                  "k_jac_ne_u<6,2,false>", 1500, 257, 0, [6], BAND, (S_CHOL,)),
    # ---- no globals, no solved bundle (C2 class): block-diagonal direct solve ----
    "c2_pc7": _s(_cfg(1, frames=12, scale=0.05), "k_ne_cf_u<7,4,0>, k_bd_direct",
                 None, 12, 0, [7], BDIAG, (S_BD,)),
    "c2_pc6": _s(_cfg(1, frames=12, scale=0.05, solve_focal=False),
                 "k_ne_cf_u<6,4,0>, k_bd_direct", None, 12, 0, [6], BDIAG, (S_BD,)),
    # ---- one or two globals, no solved bundle (C5 class) ----
    "c5_f8": _s(_cfg(4, frames=8, scale=0.05), "k_ne_cf_u<6,1,2>, k_ne_glob<2>, k_bd_root",
                None, 16, 2, [12], BDIAG, (S_BD,)),
    "c5_f4_wide": _s(_cfg(4, frames=4, scale=0.2), "k_ne_cf_glob<6>",
                     1600, 8, 2, [12], BDIAG, (S_BD,)),
    "c5_pc7": _s(_cfg(4, frames=8, scale=0.05, block_focal=True),
                 "k_ne_cf_u<7,1,2>, k_ne_glob<2>", None, 16, 2, [14], BDIAG, (S_BD,)),
    "c5_pc7_wide": _s(_cfg(4, frames=4, scale=0.2, block_focal=True), "k_ne_cf_glob<7>",
                      1600, 8, 2, [14], BDIAG, (S_BD,)),
    # 65 chunks of 512 observations: k_ne_glob_reduce's stride loop
    "c5_65chunks": _s(_cfg(4, frames=2, scale=8.2, cameras=1),
                      "k_ne_cf_glob<6> with 65 global chunks, k_ne_glob_reduce past 64",
                      32800, 2, 2, [6], BDIAG, (S_BD,)),
    "c5_wide12": _s(_cfg(4, frames=6, scale=0.05, lens_model="classic_wide", cameras=1),
                    "12-wide camera-frame blocks, k_ne_cf generic", None, 6, 0, [12], BDIAG,
                    (S_BD,)),
    # ---- witness rigs: the arrow of globals, with solved bundles (band + arrow) ----
    "wit_g4": _s(_wit(n_witness=1, n_focal=1), "k_ne_glob<4>, k_ne_cf, k_ne_bnd, k_schur_glob",
                 None, None, 4, [6], BAND, (S_CHOL,), opt="plain"),
    "wit_g5": _s(_wit(n_witness=1, n_focal=1, extra_globals=1), "k_ne_glob<8>",
                 None, None, 5, [6], BAND, (S_CHOL,), opt="plain"),
    "wit_g11": _s(_wit(n_witness=2, n_focal=2), "k_ne_glob<16>",
                  None, None, 11, [6], BAND, (S_CHOL,), opt="plain"),
    "wit_g16": _s(_wit(n_witness=3, n_focal=1, frames=4), "k_ne_glob<16> at its capacity",
                  None, None, 16, [6], BAND, (S_BCR,), opt="plain"),
    "wit_g40": _s(_wit(n_witness=6, n_focal=6, extra_globals=1, frames=4), "k_ne_glob_wide",
                  None, None, 40, [6], BAND, (S_BCR,), opt="plain"),
    # an observation with 17 / 19 columns on a plan with 14 globals
    "wit_lens_g14": _s(_wit(n_witness=1, n_focal=1, lens="anamorphic"),
                       "ne_glob_body's nl > 12 branch in k_ne_glob<16>",
                       None, None, 14, [6], BAND, (S_CHOL,), opt="plain"),
    "wit_wide_block": _s(_wit(n_witness=1, n_focal=1, wide_block=True),
                         "k_schur_obs<PCMAX>, generic k_schur_dest, 12-wide blocks",
                         None, None, 4, [12], BAND, (S_CHOL,), opt="plain"),
    # ... without a solved bundle: block diagonal + arrow
    "wit_bd_g4": _s(_wit(n_witness=1, n_focal=1, solve_bundles=False), "k_bd_root, 4 globals",
                    None, None, 4, [6], BDIAG, (S_BD,), opt="plain"),
    "wit_bd_g11": _s(_wit(n_witness=2, n_focal=2, solve_bundles=False), "k_bd_root, 11 globals",
                     None, None, 11, [6], BDIAG, (S_BD,), opt="plain"),
    "wit_bd_g16": _s(_wit(n_witness=3, n_focal=1, frames=4, solve_bundles=False),
                     "k_bd_root, 16 globals", None, None, 16, [6], BDIAG, (S_BD,), opt="plain"),
    # ---- C3 class: bundles seen by several cameras, tiled and dense solvers ----
    "c3_tiled_lane0": _s(_cfg(2, frames=4, scale=0.002), "tiled Cholesky, k_schur_dest_u<6> alone",
                         None, 40, 0, [54, 60], TILED, (S_NONE,),
                         pins={abi.PATH_DENSE: 0, abi.PATH_DEST_LANE: 0}),
    "c3_tiled_lane1": _s(_cfg(2, frames=4, scale=0.002), "tiled Cholesky, k_schur_dest_lane<6>",
                         None, 40, 0, [54, 60], TILED, (S_NONE,),
                         pins={abi.PATH_DENSE: 0, abi.PATH_DEST_LANE: 1}, same_as="c3_tiled_lane0"),
    "c3_dense": _s(_cfg(2, frames=4, scale=0.002), "dense solver",
                   None, 40, 0, [54, 60], DENSE, (S_NONE,), pins={abi.PATH_DENSE: 1},
                   same_as="c3_tiled_lane0"),
    # ---- edge scenes ----
    "edge_dup": _s(_edge(duplicate_markers=3), "pair (i, j) destinations", None, 6, 0, [6],
                   BAND, (S_BCR,), opt="plain"),
    "edge_g1": _s(_edge(static_focal=True, parented=True), "one global", None, 6, 1, [6],
                  BAND, (S_BCR,), opt="plain"),
    "edge_g3": _s(_edge(parented=True, solve_parent=True), "three globals", None, 6, 3, [6],
                  BAND, (S_BCR,), opt="plain"),
    "edge_rows": _s(_edge(stiffness=True), "attribute rows (k_rows_jac, k_rows_ne)", None, 6, 0,
                    [6], BAND, (S_BCR,), opt="plain", mode=DAG),
    "edge_rs": _s(_rs_parented, "k_schur_obs_rs, launch_ne_rs", None, 6, 0, [6], BAND, (S_BCR,),
                  opt="plain"),
}

# (scene, lam): e64 -- 1000 e64 above STEP_CAP, so the pair has no sharp bar
LEFT_OUT = {
    # frames with one or two observations: J^T J is singular without damping
    ("c4_f257", 0.0): 1.0,
    # the parent group's rotation against the camera's own: e64 = 17
    ("edge_g3", 0.0): 17.0,
    # twelve-wide blocks (focal length, film offsets / lens coefficients keyed
    # per frame): J^T J is singular without damping
    ("c5_wide12", 0.0): np.inf,
    ("wit_wide_block", 0.0): np.inf,
}

CASES = [pytest.param(name, lam, id="%s-lam%g" % (name, lam))
         for name in SCENES for lam in LAMS if (name, lam) not in LEFT_OUT]

# pins whose two settings the code describes as the same operations: the
# steps must be bit-equal (each also meets the bars).  (key, value, scene)
PIN_PAIRS = [
    pytest.param(abi.PATH_PRE_SCHUR, 1, "c4_f257", id="pre_schur"),
    pytest.param(abi.PATH_BACKSUB_ONEPASS, 1, "c4_f8", id="backsub_onepass"),
    pytest.param(abi.PATH_JB_RECOMPUTE, 1, "c4_f257", id="jb_recompute"),
    pytest.param(abi.PATH_RED_BD, 0, "c2_pc7", id="red_bd"),
    pytest.param(abi.PATH_TRIAL_RECORDS, 0, "c4_f8", id="trial_records"),
]


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name]["make"]()


def options(name):
    sc = SCENES[name]
    if sc["opt"] == "config":
        return S.config_options(scene(name), scene_graph_mode=sc["mode"])
    return make_options(scene_graph_mode=sc["mode"])


def num_globals(prob):
    bnd_attrs = set()
    for b in range(prob.num_bundles):
        t = prob.bnd_tfm[b]
        bnd_attrs.update(int(a) for a in prob.tfm_attrs[9 * t:9 * t + 3])
    return sum(1 for p in range(prob.num_params)
               if prob.param_frame[p] < 0 and int(prob.param_attr[p]) not in bnd_attrs)


def camera_frames(prob):
    cam = np.asarray(prob.mkr_cam)[prob.obs_marker]
    return len(set(zip(prob.obs_frame.tolist(), cam.tolist())))


def check_shape(name):
    """The structural facts the scene's dispatch rests on (CPU side)."""
    sc, prob = SCENES[name], scene(name)
    if sc["M"] is not None:
        assert prob.num_obs == sc["M"]
    if sc["cf"] is not None:
        assert camera_frames(prob) == sc["cf"]
    assert num_globals(prob) == sc["nG"]
    fr = prob.param_frame[prob.param_frame >= 0]
    counts = np.bincount(fr, minlength=prob.num_frames)
    assert sorted(set(counts[counts > 0].tolist())) == sc["pcs"]


# ---- the reference ----

def gram_extended(J, f, block=32):
    """A = J^T J, g = J^T f in numpy.longdouble and |J|^T |f| in fp64, formed in
    row blocks over the columns each block touches (J is sparse)."""
    assert np.finfo(np.longdouble).eps < 1e-18, "numpy.longdouble is not extended precision"
    m, n = J.shape
    A = np.zeros((n, n), np.longdouble)
    g = np.zeros(n, np.longdouble)
    for r0 in range(0, m, block):
        Jb = J[r0:r0 + block]
        cols = np.flatnonzero(np.any(Jb != 0., axis=0))
        if cols.size == 0:
            continue
        Jl = Jb[:, cols].astype(np.longdouble)
        A[np.ix_(cols, cols)] += Jl.T @ Jl
        g[cols] += Jl.T @ f[r0:r0 + block].astype(np.longdouble)
    return A, g, np.abs(J).T @ np.abs(f)


def solve_refined(Ad, g, steps=4):
    """Ad p = g: fp64 solves, refined against the extended-precision residual."""
    Ainv = np.linalg.inv(Ad.astype(np.float64))  # one factorisation for the five solves
    p = (Ainv @ g.astype(np.float64)).astype(np.longdouble)
    for _ in range(steps):
        r = g - Ad @ p
        p = p + (Ainv @ r.astype(np.float64)).astype(np.longdouble)
    return p


def step_error(p, p_ref, D):
    return float(np.max(np.abs(D * (p - p_ref))) / np.max(np.abs(D * p_ref)))


class Reference:
    """The reference of one (J, f): g, D, and per lam the step and e64."""

    def __init__(self, J, f):
        self.m = J.shape[0]
        self.A, g, self.abs_g = gram_extended(J, f)
        self.g = SIGN * g
        d2 = np.diagonal(self.A).copy()
        D = np.sqrt(d2)
        D[d2 == 0] = 1.0
        self.D = D
        # the plain fp64 evaluation of the same formula
        self.A64 = J.T @ J
        self.g64 = SIGN * (J.T @ f)
        D64 = np.sqrt(np.diagonal(self.A64))
        D64[D64 == 0.] = 1.0
        self.D64 = D64
        self._steps = {}

    def step(self, lam):
        """(p_ref, e64) at lam."""
        if lam not in self._steps:
            Ad = self.A + np.longdouble(lam) * np.diag(self.D * self.D)
            D = self.D.astype(np.float64)
            try:
                p = solve_refined(Ad, self.g).astype(np.float64)
                p64 = np.linalg.solve(self.A64 + lam * np.diag(self.D64 * self.D64), self.g64)
                self._steps[lam] = (p, step_error(p64, p, D))
            except np.linalg.LinAlgError:  # singular: no bar, the pair is not admissible
                self._steps[lam] = (np.full(D.size, np.nan), np.inf)
        return self._steps[lam]

    def step_bar(self, lam):
        return STEP_MARGIN * self.step(lam)[1]


# ---- CPU: every scene is what the table says, and can notice an error ----

@pytest.mark.parametrize("name", sorted(SCENES))
def test_scene_shape(name):
    check_shape(name)


@functools.lru_cache(maxsize=None)
def oracle_reference(name):
    from oracle import refcpu
    prob = scene(name)
    f, J = refcpu.jacobian(prob, options(name), prob.x0)
    return Reference(np.ascontiguousarray(J), f), J, f


# The oracle's FD Jacobian of these costs over half a minute on the CPU (n
# columns x M observations): their power is asserted on the device's J instead
# (test_damped_step).
SLOW_ON_CPU = {"c4_f257"}
# scenes sharing a factory share the CPU part
CPU_SCENES = sorted(n for n, sc in SCENES.items()
                    if sc["same_as"] is None and n not in SLOW_ON_CPU)


def check_power(name, J, f, ref):
    """Every (scene, lam) pair tested is admissible (1000 e64 <= 1e-7), and
    zeroing the two rows of one observation (the first, the middle and the
    last that reach a solved parameter, each alone) moves the reference step
    by at least 1000 x the step bar."""
    M = scene(name).num_obs
    # (a locked camera seeing a locked bundle has two zero rows)
    live = [i for i in range(M) if np.any(J[2 * i:2 * i + 2] != 0.)]
    lams = [lam for lam in LAMS if (name, lam) not in LEFT_OUT]
    moved = {lam: [] for lam in lams}
    for i in (live[0], live[len(live) // 2], live[-1]):
        Jz = J.copy()
        Jz[2 * i:2 * i + 2] = 0.
        rz = Reference(Jz, f)
        for lam in lams:
            moved[lam].append(step_error(rz.step(lam)[0], ref.step(lam)[0],
                                         ref.D.astype(np.float64)))
    for lam in lams:
        print("%-16s lam %-6g n %4d  e64 %.2g  bar %.2g  one observation moves the step by >= "
              "%.2g" % (name, lam, J.shape[1], ref.step(lam)[1], ref.step_bar(lam),
                        min(moved[lam])))
    for (nm, lam), e in LEFT_OUT.items():
        if nm == name:
            print("%-16s lam %-6g left out (e64 %.2g)" % (name, lam, e))
    for lam in lams:
        assert ref.step_bar(lam) <= STEP_CAP, (lam, ref.step(lam)[1])
        assert min(moved[lam]) >= 1000.0 * ref.step_bar(lam), (lam, moved[lam])


@pytest.mark.parametrize("name", CPU_SCENES)
def test_one_observation_moves_the_reference(name):
    """check_power on the oracle's J and f at x0."""
    ref, J, f = oracle_reference(name)
    check_power(name, J, f, ref)


def test_left_out_pairs():
    """Only lam = 0 is ever left out, and only where the plain fp64
    evaluation has no sharp bar (1000 e64 > 1e-7 on the oracle's J)."""
    for (name, lam), e in LEFT_OUT.items():
        assert lam == 0.0 and name in SCENES
        if name in SLOW_ON_CPU:
            continue
        ref, _J, _f = oracle_reference(name)
        assert ref.step_bar(lam) > STEP_CAP, (name, ref.step(lam)[1])


# ---- GPU ----

_runs = {}


def device_run(name, ctx, set_path, extra_pins=None):
    """One plan of the scene (its pins set while it is built): the damped step
    at x0 for every lam, the dense J of each pass, f from measure, and the
    reference built from the device's J and f.  Computed once per key."""
    key = (name, tuple(sorted((extra_pins or {}).items())))
    if key in _runs:
        return _runs[key]
    sc, prob = SCENES[name], scene(name)
    pins = dict(sc["pins"])
    pins.update(extra_pins or {})
    for k, v in pins.items():
        set_path(k, v)
    s = Solver(prob, options(name), context=ctx)
    try:
        st = s.kernel_stats()
        out = {}
        J0 = None
        for lam in LAMS:
            if (name, lam) in LEFT_OUT:
                continue
            step, g, diag, J = s.damped_step(prob.x0, lam)
            if J0 is None:
                J0 = J
            else:  # the same pass at the same x: the same J
                np.testing.assert_array_equal(J, J0)
            out[lam] = (step, g, diag)
        f = s.measure(prob.x0)[0]
    finally:
        s.close()
    run = dict(stats=st, out=out, J=J0, f=f, ref=None)
    _runs[key] = run
    return run


def reference_of(run):
    if run["ref"] is None:
        run["ref"] = Reference(run["J"], run["f"])
    return run["ref"]


def check_bars(name, lam, run, what=""):
    ref = reference_of(run)
    step, g, diag = run["out"][lam]
    p_ref, e64 = ref.step(lam)
    D = ref.D.astype(np.float64)
    m = ref.m
    g_ref = ref.g.astype(np.float64)
    g_bar = 4.0 * m * EPS * ref.abs_g
    g_err = float(np.max(np.abs(g - g_ref) / np.maximum(g_bar, np.finfo(float).tiny)))
    d_err = float(np.max(np.abs(diag - D) / (4.0 * m * EPS * D)))
    err = step_error(step, p_ref, D)
    print("%-16s%s lam %-6g n %4d m %6d  e64 %.2g  bar %.2g  device %.2g  (g %.2g, D %.2g of "
          "their bars)" % (name, what, lam, D.size, m, e64, ref.step_bar(lam), err, g_err, d_err))
    assert np.all(np.isfinite(step)) and np.all(np.isfinite(g)) and np.all(np.isfinite(diag))
    assert ref.step_bar(lam) <= STEP_CAP_DEVICE, "no sharp bar on this J: e64 %.3g" % e64
    assert np.all(np.abs(g - g_ref) <= g_bar), "g: %.3g of its bar" % g_err
    assert np.all(np.abs(diag - D) <= 4.0 * m * EPS * D), "D: %.3g of its bar" % d_err
    assert err <= ref.step_bar(lam), "step: %.3g against %.3g" % (err, ref.step_bar(lam))


def check_stats(name, st):
    sc = SCENES[name]
    assert st["reduced_kind"] == sc["kind"], st
    if sc["solver"] is not None:
        assert st["band_solver"] in sc["solver"], st
    prob = scene(name)
    n_blocks = int(np.sum(prob.param_frame >= 0)) + sc["nG"]
    assert st["reduced_dim"] == n_blocks, st


@gpu
@pytest.mark.parametrize("name,lam", CASES)
def test_damped_step(name, lam, gpu_ctx, paths):
    """g, D and the damped step of mmba_debug_damped_step at x0 against the
    extended-precision reference of the device's own J and f, at the bars of
    the module docstring."""
    check_shape(name)
    run = device_run(name, gpu_ctx, paths)
    check_stats(name, run["stats"])
    check_bars(name, lam, run)
    if name in SLOW_ON_CPU and lam == LAMS[0]:
        check_power(name, run["J"], run["f"], reference_of(run))


@gpu
@pytest.mark.parametrize("key,value,name", PIN_PAIRS)
def test_pinned_pairs_bit_equal(key, value, name, gpu_ctx, paths):
    """A path pin whose two settings run the same operations: the steps, g
    and D of the pinned plan are bit-equal to the default plan's at every
    lam, besides meeting the bars.  (PATH_PRE_SCHUR acts on the Jacobian a
    solve enqueues ahead of its decision, which the hook does not do: that
    pair holds by construction.)"""
    base = device_run(name, gpu_ctx, paths)
    for k in range(1, abi.PATH_NUM):
        paths(k, -1)
    run = device_run(name, gpu_ctx, paths, {key: value})
    np.testing.assert_array_equal(run["J"], base["J"])
    for lam in run["out"]:
        check_bars(name, lam, run, " pin %d=%d" % (key, value))
        for a, b, what in zip(run["out"][lam], base["out"][lam], ("step", "g", "D")):
            np.testing.assert_array_equal(a, b, err_msg="%s at lam %g" % (what, lam))


@gpu
def test_hook_refusals(gpu_ctx):
    """lam < 0 is invalid; a second call on the same plan repeats the first
    bit for bit (nothing the hook leaves behind changes the next call)."""
    from mayamatchmovesolver_amd._lib import MmbaError
    prob = scene("c4_f8")
    s = Solver(prob, options("c4_f8"), context=gpu_ctx)
    try:
        with pytest.raises(MmbaError):
            s.damped_step(prob.x0, -1.0)
        a = s.damped_step(prob.x0, 1e-3)
        s.solve()
        b = s.damped_step(prob.x0, 1e-3)
        for u, v in zip(a, b):
            np.testing.assert_array_equal(u, v)
    finally:
        s.close()
