"""The damped LM step of B15 plans against a dense reference.

lmder with central differences over animated parameters of several frames
builds a B15 plan (Plan::build): the reference's Jacobian is J = J_s + f c^T,
and the device carries the rank-one term through a per-camera-frame
Householder basis (k_b15_q, k_b15_rot, k_b15_accl, k_b15_unrot,
k_b15_unrot_J), two damped solves of M = J_s^T J_s + lam Q D^2 Q, a 2 x 2
Woodbury combine (k_b15_combine) and its own ||D p|| (k_b15_dnorm).
mmba_debug_damped_step hands back the step, g = J^T f, D and the dense J in
the original basis and parameter order; helpers, bars and margins are those
of test_gpu_damped_step.py.

The split, from the dense J and f alone: every row j of another frame than an
animated parameter p's holds exactly f_j c_p, so c_p is read off those rows
(only rows with |f_j| >= 1e-3 max|f|; they must agree within 8 eps relative),
J_s := J - f c^T on the parameter's own frame and 0 elsewhere; static columns
have c = 0.

Reference: A = J^T J and g = J^T f of J = J_s + f c^T in numpy.longdouble
(the sparse J_s^T J_s and u = J_s^T f by gram_extended, then u c^T + c u^T +
s c c^T and u + s c, s = f^T f, all in longdouble: the same sums as the dense
product, without forming it), D = sqrt(diag A) (1 for a zero column),
(A + lam D^2) p = g by solve_refined.

Bars (m = rows of J, eps = 2^-52):
  g     |g - g_ref| <= 4 m eps (|J|^T |f|)   componentwise
  D     |D - D_ref| <= 4 m eps D_ref
  step  max|D (p - p_ref)| / max|D p_ref| <= 1000 e64rot
e64rot is the same measure of the step numpy computes in plain fp64 by the
formulation the plan documents (mmba_plan.h at Plan::b15, mmba_kernels.hip
"B15: ... A = M + U B U^T"), written out in rotated_step below: the animated
columns are nearly parallel to f, so the plain original-basis e64 is a weak
yardstick here (it grows like 1 / lam) and is only printed beside e64rot.  A
(scene, lam) pair is admissible only if 1000 e64rot <= 1e-7 on the oracle's J
and zeroing one observation's two rows moves the reference step by at least
1000 x that bar (test_one_observation_moves_the_reference); on the device's J
the bar may reach 1e-6 (STEP_CAP_DEVICE).

Scenes (all auto_diff_type = CENTRAL; kind / solver asserted from
mmba_kernel_stats).  The damped solve of a B15 plan runs
Plan::solve_damped_enqueue twice with dnorm_slot = -1, so the block-diagonal
plans (b15_c2_*) take k_schur_init + bd_factor_solve there, not the one-launch
k_bd_direct the non-B15 C2 plans of test_gpu_damped_step.py take.

Pairs left out, by name, in LEFT_OUT_B15 with the figure that fails:
lam = 0 everywhere (1000 e64rot > 1e-7), lam = 1e-3 on the two C2 scenes (one
observation moves the step by less than 1000 x the bar) and lam = 1e-6 on
b15_c4_f32_pcr (1000 e64rot > 1e-7).  test_left_out_pairs asserts each.

Not reached: lam = 0 on B15 plans; k_b15_newton and k_b15_jp (lmpar's Newton
term and ||J p||: scalars the hook does not return, held by test_gpu_b15.py's
trace parity only).

Measured on an MI355X, e64 / e64rot / the device's error (the step measure, on
the device's J; g and D stayed below 2.0e-3 of their bars everywhere; every
run prints these lines with -s):

scene              n     m  lam 1                         lam 1e-3                      lam 1e-6
b15_c4_f8        189   400  1.3e-14 / 8.8e-15 / 3.3e-15   9.6e-12 / 3.2e-13 / 1.2e-13   1.1e-08 / 2.5e-11 / 2.6e-11
b15_c4_f8_pcr    189   400  1.3e-14 / 8.8e-15 / 3.3e-15   9.6e-12 / 3.2e-13 / 1.2e-13   1.1e-08 / 2.5e-11 / 2.6e-11
b15_c4_f8_bcr    189   400  1.3e-14 / 8.8e-15 / 3.3e-15   9.6e-12 / 3.2e-13 / 9.7e-14   1.1e-08 / 2.5e-11 / 2.6e-11
b15_c4_f32_pcr   633  1200  1.4e-13 / 1.2e-14 / 6.9e-15   9.2e-11 / 3.7e-12 / 2.3e-13   left out (bar)
b15_edge          99   288  1e-14 / 1.9e-15 / 1.3e-15     7.9e-12 / 4.9e-13 / 3.1e-14   3e-09 / 4e-12 / 3.3e-12
b15_edge_dag      99   288  1.4e-14 / 2.5e-15 / 2.1e-15   8.5e-12 / 1.3e-13 / 1.4e-13   3.1e-09 / 6.7e-12 / 2.7e-12
b15_edge_g1      100   288  1.1e-14 / 7e-15 / 1.6e-15     3.9e-12 / 8.6e-14 / 4.1e-14   4.8e-10 / 4.5e-13 / 5.6e-13
b15_edge_par4     87   192  4.4e-15 / 2.7e-15 / 8.7e-16   3.4e-12 / 8.8e-14 / 7e-14     1.1e-09 / 1.4e-12 / 1.4e-12
b15_edge_f9       81   216  2.2e-14 / 7.3e-15 / 2.9e-15   1.2e-11 / 1.9e-13 / 4.3e-14   5.2e-09 / 9.3e-12 / 8.6e-12
b15_c2_pc7        56   320  2.4e-14 / 5.9e-15 / 2.8e-15   left out (power)              2.2e-08 / 8.1e-12 / 8.5e-12
b15_c2_pc6        48   320  1.9e-14 / 2e-15 / 2.5e-15     left out (power)              1.9e-08 / 6.8e-12 / 7e-12

The largest device error is 1.3 x e64rot (b15_c2_pc6 at lam = 1, b15_edge_g1
at lam = 1e-6), against the margin of 1000.  The rotated basis gains what
e64 / e64rot says: 1.5 to 12 at lam = 1, 16 to 65 at lam = 1e-3 and 440 to
2,800 at lam = 1e-6 (2.5 to 3.5 digits; at lam = 0, on the oracle's J, 230 to
89,000, up to 5 digits), growing like 1 / lam as the damping stops hiding the
animated columns' common direction f.

Scratch builds, one slip each, the same cases (arithmetic only):
  k_b15_combine with cc = -be for s - be: step errors of 6.9 to 1.5e4 against
    bars of 1.9e-12 to 2.5e-8; all 30 cases fail;
  k_b15_accl adding lam D^2 unrotated for lam Q D^2 Q: step errors of 1.0e-9
    to 8.8e-8 (the D of one block's columns differ little); the 25 cases with
    a bar below that fail, b15_c4_f8* and b15_c2_* at lam = 1e-6 (bars 2.5e-8,
    8.1e-9, 6.8e-9 against 4.0e-9, 1.1e-9, 1.0e-9) do not;
  the hook returning d_g (the rotated u) for d_g15: g stands 9.4e11 to 5.9e12 x
    above its bar on every scene, the step unchanged; all 30 cases fail.
"""
import functools

import numpy as np
import pytest

from mayamatchmovesolver_amd import abi, make_options, synthetic as S
from mayamatchmovesolver_amd.solver import Solver

from test_gpu_damped_step import (BAND, BDIAG, DAG, EPS, MMSG, S_BCR, S_BD, S_CHOL, S_PCR, S_PCRI,
                                  SIGN, STEP_CAP, STEP_CAP_DEVICE, Reference,
                                  camera_frames, gram_extended, num_globals, solve_refined,
                                  step_error)

gpu = pytest.mark.gpu

CENTRAL = abi.AUTO_DIFF_TYPE_CENTRAL
LAMS_B15 = [1.0, 1e-3, 1e-6]
C_AGREE = 8.0 * EPS      # the rows that carry f_j c_p agree on c_p within this, relative
F_FLOOR = 1e-3           # ... among rows with |f_j| >= F_FLOOR max|f|
POWER = 1000.0           # one observation moves the reference step by >= POWER x the bar


def _cfg(index, **kw):
    return lambda: S.make_config(index, **kw)


def _edge(**kw):
    return lambda: S.edge_scene(**kw)


# name: factory, what the scene is here for, M observations, cf camera-frames,
# nG globals, pcs = the distinct per-frame solved parameter counts, kind /
# solver of mmba_kernel_stats (Plan::build: the band solvers as on the forward
# plans of the same scenes; without a solved bundle the block-diagonal kind),
# options ("config": synthetic.config_options, else make_options), scene-graph
# mode, path pins.
def _s(make, reaches, M, cf, nG, pcs, kind, solver, opt="config", mode=MMSG, pins=None,
       same_as=None):
    return dict(make=make, reaches=reaches, M=M, cf=cf, nG=nG, pcs=pcs, kind=kind,
                solver=solver, opt=opt, mode=mode, pins=pins or {}, same_as=same_as)


_C4_F8 = _cfg(3, frames=8, scale=0.001)
SCENES = {
    "b15_c4_f8": _s(_C4_F8, "band, default solver", 200, 8, 0, [6], BAND, (S_PCR, S_PCRI)),
    "b15_c4_f8_pcr": _s(_C4_F8, "band, parallel cyclic reduction", 200, 8, 0, [6], BAND,
                        (S_PCR, S_PCRI), pins={abi.PATH_PCR: 1}, same_as="b15_c4_f8"),
    "b15_c4_f8_bcr": _s(_C4_F8, "band, block cyclic reduction", 200, 8, 0, [6], BAND, (S_BCR,),
                        pins={abi.PATH_PCR: 0}, same_as="b15_c4_f8"),
    # (scale 0.003, 600 observations: at c4_f32_pcr's 0.004 one observation moved
    # the lam = 1e-3 reference step by 938 x the bar here, short of the 1000 x
    # asked; at 0.003 by 9.5e3 x)
    "b15_c4_f32_pcr": _s(_cfg(3, frames=32, scale=0.003, window=4, depth=(4, 10)),
                         "parallel cyclic reduction, five levels; n = 633", 600, 32, 0, [6],
                         BAND, (S_PCR, S_PCRI), pins={abi.PATH_PCR: 1}),
    # every bundle is seen on every frame, so the reduced camera system is full:
    # five solved frames give bw 29, K = 32 -- block cyclic reduction
    "b15_edge": _s(_edge(), "the small case", 144, 6, 0, [6], BAND, (S_BCR,), opt="plain"),
    "b15_edge_dag": _s(_edge(), "... in the other scene graph", 144, 6, 0, [6], BAND, (S_BCR,),
                       opt="plain", mode=DAG, same_as="b15_edge"),
    "b15_edge_g1": _s(_edge(static_focal=True), "one global: the arrow, c = 0 on a global",
                      144, 6, 1, [6], BAND, (S_BCR,), opt="plain"),
    # three solved frames: bw 17, K = 24 and no arrow -- parallel cyclic reduction
    "b15_edge_par4": _s(_edge(parented=True, frames=4), "parented camera", 96, 4, 0, [6], BAND,
                        (S_PCR, S_PCRI), opt="plain", mode=DAG),
    # eight solved frames: bw 47 > 32 -- the band Cholesky
    "b15_edge_f9": _s(_edge(frames=9, bundles=12, seed=21), "odd frame count; band Cholesky",
                      108, 9, 0, [6], BAND, (S_CHOL,), opt="plain"),
    # no solved bundle: the block-diagonal reduced solve, whose inner solves
    # (dnorm_slot = -1) run k_schur_init + bd_factor_solve
    "b15_c2_pc7": _s(_cfg(1, frames=8, scale=0.004), "block-diagonal reduced solve, 7-wide",
                     160, 8, 0, [7], BDIAG, (S_BD,)),
    "b15_c2_pc6": _s(_cfg(1, frames=8, scale=0.004, solve_focal=False),
                     "block-diagonal reduced solve, 6-wide", 160, 8, 0, [6], BDIAG, (S_BD,)),
}

# (scene, lam): (which condition fails, the figure measured on the oracle's J)
#   "bar":   1000 e64rot > 1e-7; the figure is e64rot
#   "power": one observation moves the reference step by less than 1000 x the
#            bar; the figure is that ratio (moved / bar)
LEFT_OUT_B15 = {
    ("b15_c4_f8", 0.0): ("bar", 9.4e-7),
    ("b15_c4_f8_pcr", 0.0): ("bar", 9.4e-7),
    ("b15_c4_f8_bcr", 0.0): ("bar", 9.4e-7),
    ("b15_c4_f32_pcr", 0.0): ("bar", 3.8e-6),
    ("b15_edge", 0.0): ("bar", 5.7e-9),
    ("b15_edge_dag", 0.0): ("bar", 5.8e-9),
    ("b15_edge_g1", 0.0): ("bar", 2.9e-9),
    ("b15_edge_par4", 0.0): ("bar", 1.8e-10),
    ("b15_edge_f9", 0.0): ("bar", 8.6e-9),
    ("b15_c2_pc7", 0.0): ("bar", 1.3e-6),
    ("b15_c2_pc6", 0.0): ("bar", 6.7e-8),
    # bars 4.5e-9 / 3.1e-9, one observation moves the step by 1.1e-6 / 1.0e-6
    ("b15_c2_pc7", 1e-3): ("power", 2.4e2),
    ("b15_c2_pc6", 1e-3): ("power", 3.2e2),
    # one step from undamped on 633 parameters: the bar would be 1.4e-7
    ("b15_c4_f32_pcr", 1e-6): ("bar", 1.4e-10),
}

CASES = [pytest.param(name, lam, id="%s-lam%g" % (name, lam))
         for name in SCENES for lam in LAMS_B15 if (name, lam) not in LEFT_OUT_B15]


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name]["make"]()


def options(name):
    sc = SCENES[name]
    if sc["opt"] == "config":
        return S.config_options(scene(name), scene_graph_mode=sc["mode"], auto_diff_type=CENTRAL)
    return make_options(scene_graph_mode=sc["mode"], auto_diff_type=CENTRAL)


def lams_of(name):
    return [lam for lam in LAMS_B15 if (name, lam) not in LEFT_OUT_B15]


def check_shape(name):
    """The structural facts the scene's dispatch rests on (CPU side), and what
    makes it a B15 plan: animated parameters on more than one frame."""
    sc, prob = SCENES[name], scene(name)
    assert prob.num_obs == sc["M"]
    assert prob.num_residuals == 2 * prob.num_obs  # no attribute rows (Plan::build refuses them)
    assert camera_frames(prob) == sc["cf"]
    assert num_globals(prob) == sc["nG"]
    fr = prob.param_frame[prob.param_frame >= 0]
    counts = np.bincount(fr, minlength=prob.num_frames)
    assert sorted(set(counts[counts > 0].tolist())) == sc["pcs"]
    assert np.count_nonzero(counts) > 1


# ---- the split and the reference ----

def frame_blocks(prob):
    """The animated parameters of each frame, in parameter order (one camera:
    a frame's animated parameters are one camera-frame block)."""
    pf = np.asarray(prob.param_frame)
    return [np.flatnonzero(pf == k) for k in sorted(set(pf[pf >= 0].tolist()))]


def split(J, f, prob):
    """(J_s, c, spread) with J = J_s + f c^T: c_p from the rows of the other
    frames (|f_j| >= F_FLOOR max|f|), spread = the largest relative
    disagreement of those rows on any c_p."""
    J = np.asarray(J)
    pf = np.asarray(prob.param_frame)
    row_frame = np.repeat(np.asarray(prob.obs_frame), 2)
    assert J.shape[0] == row_frame.size == f.size
    big = np.abs(f) >= F_FLOOR * np.max(np.abs(f))
    Js = np.array(J, dtype=np.float64, order="C")
    c = np.zeros(J.shape[1])
    spread = 0.0
    for p in np.flatnonzero(pf >= 0):
        other = row_frame != pf[p]
        rows = big & other
        assert np.count_nonzero(rows) >= 2, "parameter %d: no row to read c from" % p
        est = J[rows, p] / f[rows]
        c[p] = np.median(est)
        assert c[p] != 0.
        spread = max(spread, float((est.max() - est.min()) / abs(c[p])))
        Js[:, p] = np.where(other, 0., J[:, p] - f * c[p])
    return Js, c, spread


def householder(c, blocks):
    """Q (n x n, block diagonal, symmetric orthogonal) with Q c_blk = kappa e_0
    per block -- v = c_blk + sign(c_0) |c_blk| e_0, Q = I - 2 v v^T / v^T v,
    kappa = -sign(c_0) |c_blk|, Q = I where c_blk = 0 (k_b15_q) -- and c in
    that basis: kappa at the block's first parameter, 0 elsewhere."""
    n = c.size
    Q = np.eye(n)
    cr = c.copy()
    for idx in blocks:
        v = c[idx].copy()
        nrm = np.sqrt(v @ v)
        if nrm == 0.:
            continue
        sg = -1.0 if v[0] < 0. else 1.0
        v[0] += sg * nrm
        Q[np.ix_(idx, idx)] = np.eye(idx.size) - (2.0 / (v @ v)) * np.outer(v, v)
        cr[idx] = 0.
        cr[idx[0]] = -sg * nrm
    return Q, cr


class ReferenceB15(Reference):
    """The reference of one (J_s, c, f): g, D, and per lam the step, e64rot
    (step()[1], so step_bar is 1000 e64rot) and the plain e64."""

    def __init__(self, Js, c, f, blocks):
        self.m = Js.shape[0]
        self.Js, self.c, self.f, self.blocks = Js, c, f, blocks
        As, u, _ = gram_extended(Js, f)
        cl, fl = c.astype(np.longdouble), f.astype(np.longdouble)
        s = fl @ fl
        self.A = As + np.outer(u, cl) + np.outer(cl, u) + s * np.outer(cl, cl)
        self.g = SIGN * (u + s * cl)
        d2 = np.diagonal(self.A).copy()
        D = np.sqrt(d2)
        D[d2 == 0] = 1.0
        self.D = D
        # the plain fp64 evaluation in the original basis
        J = Js + np.outer(f, c)
        self.abs_g = np.abs(J).T @ np.abs(f)
        self.A64 = J.T @ J
        self.g64 = SIGN * (J.T @ f)
        D64 = np.sqrt(np.diagonal(self.A64))
        D64[D64 == 0.] = 1.0
        self.D64 = D64
        self._steps, self._e64 = {}, {}

    def rotated_step(self, lam):
        """The step in plain fp64 as the plan documents it: J_r = J_s Q,
        M = J_r^T J_r + lam Q D^2 Q with D^2_p = A_pp + 2 c_p u_p + s c_p^2
        (k_jac_epilogue), z_u = M^-1 u, z_c = M^-1 (Q c), K = B^-1 + U^T M^-1 U
        with U = [u c], B^-1 = [-s 1; 1 0], xs = (1 - al) z_u + (s - be) z_c
        where (al, be) = K^-1 U^T (z_u + s z_c) (k_b15_combine), p = Q xs."""
        Js, c, f = self.Js, self.c, self.f
        Q, cr = householder(c, self.blocks)
        Jr = Js @ Q
        ur = Jr.T @ f
        s = f @ f
        u = Q @ ur  # J_s^T f in the original basis (k_b15_unrot)
        app = np.einsum("ij,ij->j", Js, Js)
        d2 = np.maximum(app + 2.0 * c * u + s * c * c, 0.)
        d2[d2 == 0.] = 1.0
        M = Jr.T @ Jr + lam * (Q * d2) @ Q
        zu = np.linalg.solve(M, ur)
        zc = np.linalg.solve(M, cr)
        d00, d01, d10, d11 = ur @ zu, ur @ zc, cr @ zu, cr @ zc
        K = np.array([[d00 - s, 1.0 + d01], [1.0 + d10, d11]])
        al, be = np.linalg.solve(K, np.array([d00 + s * d01, d10 + s * d11]))
        return Q @ ((1.0 - al) * zu + (s - be) * zc)

    def step(self, lam):
        """(p_ref, e64rot) at lam."""
        if lam not in self._steps:
            Ad = self.A + np.longdouble(lam) * np.diag(self.D * self.D)
            D = self.D.astype(np.float64)
            try:
                p = solve_refined(Ad, self.g).astype(np.float64)
                self._steps[lam] = (p, step_error(SIGN * self.rotated_step(lam), p, D))
            except np.linalg.LinAlgError:  # singular: no bar, the pair is not admissible
                self._steps[lam] = (np.full(D.size, np.nan), np.inf)
        return self._steps[lam]

    def e64(self, lam):
        """The plain fp64 original-basis evaluation's error (printed only)."""
        if lam not in self._e64:
            p, _ = self.step(lam)
            try:
                p64 = np.linalg.solve(self.A64 + lam * np.diag(self.D64 * self.D64), self.g64)
                self._e64[lam] = step_error(p64, p, self.D.astype(np.float64))
            except np.linalg.LinAlgError:
                self._e64[lam] = np.inf
        return self._e64[lam]


def reference_from(J, f, prob):
    """The split of (J, f), held to C_AGREE, and its reference."""
    Js, c, spread = split(J, f, prob)
    assert spread <= C_AGREE, "rows disagree on c: %.3g" % spread
    return ReferenceB15(Js, c, np.asarray(f, dtype=np.float64), frame_blocks(prob))


# ---- CPU: every scene is what the table says, and can notice an error ----

@pytest.mark.parametrize("name", sorted(SCENES))
def test_scene_shape(name):
    check_shape(name)


@functools.lru_cache(maxsize=None)
def oracle_jacobian(name):
    from oracle import refcpu
    prob = scene(name)
    f, J = refcpu.jacobian(prob, options(name), prob.x0)
    return np.ascontiguousarray(J), f


@functools.lru_cache(maxsize=None)
def oracle_reference(name):
    J, f = oracle_jacobian(name)
    return reference_from(J, f, scene(name)), J, f


# scenes sharing a factory and a scene graph share the CPU part (the DAG twin
# of b15_edge has an oracle J of its own)
CPU_SCENES = sorted(n for n, sc in SCENES.items() if sc["same_as"] is None or sc["mode"] == DAG)


@pytest.mark.parametrize("name", CPU_SCENES)
def test_split_is_exact(name):
    """On the oracle's J: the rows of the other frames agree on c_p within 8
    eps, c = 0 exactly on every static column, J_s is confined to each
    animated parameter's own frame, and J_s + f c^T gives J back to rounding
    (two roundings of the larger of |J| and |f c^T| per entry)."""
    J, f = oracle_jacobian(name)
    prob = scene(name)
    Js, c, spread = split(J, f, prob)
    print("%-16s c agrees across rows within %.2g (bar %.2g)" % (name, spread, C_AGREE))
    assert spread <= C_AGREE
    pf = np.asarray(prob.param_frame)
    assert np.all(c[pf < 0] == 0.) and np.all(c[pf >= 0] != 0.)
    np.testing.assert_array_equal(Js[:, pf < 0], J[:, pf < 0])
    row_frame = np.repeat(np.asarray(prob.obs_frame), 2)
    for p in np.flatnonzero(pf >= 0):
        assert not np.any(Js[row_frame != pf[p], p])
    fc = np.outer(f, c)
    back = Js + fc
    assert np.all(np.abs(back - J) <= C_AGREE * np.maximum(np.abs(J), np.abs(fc)))


def moved_by_one_observation(name, ref):
    """Per lam of LAMS_B15: how far zeroing the two rows of one observation
    (the first, the middle and the last that reach a solved parameter, each
    alone) moves the reference step, at the least.  (A zeroed row of
    J = J_s + f c^T is a zeroed row of J_s and of the f in the rank-one term;
    J^T f does not see the f of a zero row, so f is zeroed throughout.)"""
    M = scene(name).num_obs
    live = [i for i in range(M) if np.any(ref.Js[2 * i:2 * i + 2] != 0.)]
    moved = {lam: [] for lam in LAMS_B15}
    D = ref.D.astype(np.float64)
    for i in (live[0], live[len(live) // 2], live[-1]):
        Jz, fz = ref.Js.copy(), ref.f.copy()
        Jz[2 * i:2 * i + 2] = 0.
        fz[2 * i:2 * i + 2] = 0.
        rz = ReferenceB15(Jz, ref.c, fz, ref.blocks)
        for lam in LAMS_B15:
            Ad = rz.A + np.longdouble(lam) * np.diag(rz.D * rz.D)
            pz = solve_refined(Ad, rz.g).astype(np.float64)
            moved[lam].append(step_error(pz, ref.step(lam)[0], D))
    return {lam: min(v) for lam, v in moved.items()}


@functools.lru_cache(maxsize=None)
def oracle_power(name):
    return moved_by_one_observation(name, oracle_reference(name)[0])


@pytest.mark.parametrize("name", CPU_SCENES)
def test_one_observation_moves_the_reference(name):
    """On the oracle's J and f at x0: every (scene, lam) pair tested is
    admissible (1000 e64rot <= 1e-7) and zeroing one observation's two rows
    moves the reference step by at least 1000 x the step bar."""
    ref, J, _f = oracle_reference(name)
    moved = oracle_power(name)
    for lam in LAMS_B15 + [0.0]:
        out = "" if lam in lams_of(name) else "  left out"
        print("%-16s lam %-6g n %4d m %5d  e64 %.2g  e64rot %.2g  bar %.2g  one observation "
              "moves the step by >= %s%s"
              % (name, lam, J.shape[1], J.shape[0], ref.e64(lam), ref.step(lam)[1],
                 ref.step_bar(lam), "%.2g" % moved[lam] if lam in moved else "-", out))
    for lam in lams_of(name):
        assert ref.step_bar(lam) <= STEP_CAP, (lam, ref.step(lam)[1])
        assert moved[lam] >= POWER * ref.step_bar(lam), (lam, moved[lam], ref.step_bar(lam))


def test_left_out_pairs():
    """lam = 0 is left out on every scene; beyond that only pairs that fail a
    condition on the oracle's J are, each for the reason LEFT_OUT_B15 names."""
    assert 0.0 not in LAMS_B15
    for name in SCENES:
        assert (name, 0.0) in LEFT_OUT_B15
    for (name, lam), (why, _figure) in LEFT_OUT_B15.items():
        assert name in SCENES and (lam == 0.0 or lam in LAMS_B15)
        base = name if name in CPU_SCENES else SCENES[name]["same_as"]
        ref, _J, _f = oracle_reference(base)
        if why == "bar":
            assert ref.step_bar(lam) > STEP_CAP, (name, lam, ref.step(lam)[1])
        else:
            assert why == "power" and ref.step_bar(lam) <= STEP_CAP
            assert oracle_power(base)[lam] < POWER * ref.step_bar(lam), (name, lam)


# ---- GPU ----

_runs = {}


def device_run(name, ctx, set_path):
    """One plan of the scene (its pins set while it is built): the damped step
    at x0 for every lam (J bit-equal across the calls), f from measure, and
    the reference built from the device's J and f.  Computed once per scene."""
    if name in _runs:
        return _runs[name]
    sc, prob = SCENES[name], scene(name)
    for k, v in sc["pins"].items():
        set_path(k, v)
    s = Solver(prob, options(name), context=ctx)
    try:
        st = s.kernel_stats()
        out = {}
        J0 = None
        for lam in lams_of(name):
            step, g, diag, J = s.damped_step(prob.x0, lam)
            if J0 is None:
                J0 = np.ascontiguousarray(J)
            else:  # the same pass at the same x: the same J
                np.testing.assert_array_equal(J, J0)
            out[lam] = (step, g, diag)
        f = s.measure(prob.x0)[0]
    finally:
        s.close()
    run = dict(stats=st, out=out, J=J0, f=f, ref=None)
    _runs[name] = run
    return run


def reference_of(name, run):
    if run["ref"] is None:
        run["ref"] = reference_from(run["J"], run["f"], scene(name))
    return run["ref"]


def check_bars(name, lam, run):
    ref = reference_of(name, run)
    step, g, diag = run["out"][lam]
    p_ref, e64rot = ref.step(lam)
    D = ref.D.astype(np.float64)
    m = ref.m
    g_ref = ref.g.astype(np.float64)
    g_bar = 4.0 * m * EPS * ref.abs_g
    g_err = float(np.max(np.abs(g - g_ref) / np.maximum(g_bar, np.finfo(float).tiny)))
    d_err = float(np.max(np.abs(diag - D) / (4.0 * m * EPS * D)))
    err = step_error(step, p_ref, D)
    print("%-16s lam %-6g n %4d m %5d  e64 %.2g  e64rot %.2g  bar %.2g  device %.2g  (g %.2g, "
          "D %.2g of their bars)" % (name, lam, D.size, m, ref.e64(lam), e64rot,
                                     ref.step_bar(lam), err, g_err, d_err))
    assert np.all(np.isfinite(step)) and np.all(np.isfinite(g)) and np.all(np.isfinite(diag))
    assert ref.step_bar(lam) <= STEP_CAP_DEVICE, "no sharp bar on this J: e64rot %.3g" % e64rot
    assert np.all(np.abs(g - g_ref) <= g_bar), "g: %.3g of its bar" % g_err
    assert np.all(np.abs(diag - D) <= 4.0 * m * EPS * D), "D: %.3g of its bar" % d_err
    assert err <= ref.step_bar(lam), "step: %.3g against %.3g" % (err, ref.step_bar(lam))


def check_stats(name, st):
    sc, prob = SCENES[name], scene(name)
    assert st["reduced_kind"] == sc["kind"], st
    assert st["band_solver"] in sc["solver"], st
    assert st["reduced_dim"] == int(np.sum(prob.param_frame >= 0)) + sc["nG"], st


@gpu
@pytest.mark.parametrize("name,lam", CASES)
def test_damped_step_b15(name, lam, gpu_ctx, paths):
    """g, D and the damped step of mmba_debug_damped_step on a B15 plan at x0
    against the extended-precision reference of the device's own J and f, at
    the bars of the module docstring."""
    check_shape(name)
    run = device_run(name, gpu_ctx, paths)
    check_stats(name, run["stats"])
    check_bars(name, lam, run)


@gpu
@pytest.mark.parametrize("name", ["b15_c4_f8", "b15_edge_g1", "b15_c2_pc7"])
def test_b15_hook_repeats(name, gpu_ctx):
    """Hook, solve(), hook again on one plan: the second call repeats the
    first bit for bit (the swaps of the damped solve and the in-place
    un-rotation of the stored J leave nothing behind), and the solve() after
    a hook call returns the bits of a fresh plan's solve()."""
    prob = scene(name)
    sc = SCENES[name]
    kw = dict(scene_graph_mode=sc["mode"], auto_diff_type=CENTRAL, iterations=20)
    opt = S.config_options(prob, **kw) if sc["opt"] == "config" else make_options(**kw)
    s = Solver(prob, opt, context=gpu_ctx)
    try:
        a = s.damped_step(prob.x0, 1e-3)
        after = s.solve()
        b = s.damped_step(prob.x0, 1e-3)
    finally:
        s.close()
    s = Solver(prob, opt, context=gpu_ctx)
    try:
        fresh = s.solve()
    finally:
        s.close()
    for u, v, what in zip(a, b, ("step", "g", "D", "J")):
        np.testing.assert_array_equal(u, v, err_msg=what)
    np.testing.assert_array_equal(after.x, fresh.x)
    np.testing.assert_array_equal(after.fnorm_trace, fresh.fnorm_trace)
    # (trial points were evaluated: their ||f|| depend on the solve's steps; on
    # b15_c2_pc7 the reference itself accepts none of them and returns x0)
    assert len(fresh.fnorm_trace) > 1
