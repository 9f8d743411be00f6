"""The reduced-system band solvers on systems whose deep levels matter.

Parallel cyclic reduction (PCR, csrc/mmba_pcr.hip) and block cyclic reduction
(BCR, csrc/mmba_bcr.hip) eliminate in ceil(log2 nblk) levels; at level l block
j meets blocks j +- 2^l.  On the diagonally dominant matrices of
test_gpu_band.py block j does not depend on block j +- 2^l beyond l = 2 at any
precision the test can see: with the right-hand side ones on block 0 the
solution on the last of 65 blocks is 6e-126 of the largest entry
(test_dominant_generator_has_no_far_field), so an error at a deep level -- a
wrong neighbour, a transposed X3, a wrong granule offset -- passes there.

chain_band_spd builds S = F F^T from a lower-triangular band factor whose rows
sum to zero (F[i, i] = 1, F[i, i-k:i] = -a, a > 0, sum a = 1), scaled to unit
diagonal plus mu = 1e-6: F^-1 does not decay, so every block depends on every
other (far field 2e-4 .. 2e-1), at condition numbers up to 4e5.  The
off-diagonal blocks of S are not symmetric, so a P / Q or L / U swap shows.

Reference (tests/test_gpu_damped_step.py's form): x_ref is an fp64 solve with
four steps of iterative refinement against the numpy.longdouble residual;
e64 is the largest max|x64 - x_ref| / max|x_ref| of the plain
numpy.linalg.solve over the case's right-hand sides (four random ones, ones
on block 0 only, ones on the last block only).

Bars, from the reference alone (n = nb + nG, eps = 2^-52):
  x    max|x - x_ref| / max|x_ref| <= bar = 1000 max(e64, n eps) for every
       right-hand side (1000 = the damped-step tests' STEP_MARGIN: another
       summation order and a multi-stage elimination; the n eps floor because
       one e64 can come out luckily small)
  yn   |yn - r.x_ref| <= bar_y |r.x_ref|, bar_y the same from the fp64 r.x64
The CPU tests (not marked gpu) hold every case to: S symmetric with half
bandwidth exactly w; every first sub-diagonal block L_j with
max|L_j - L_j^T| >= 0.01; bar <= 1e-7 (STEP_CAP); and, from two blocks on,
far >= 1000 bar, where far is the smaller of max|x| on the last block over
max|x| for ones on block 0 and the same the other way round: an error that
cuts or corrupts any level stands 1000 x above the bar.

Every PCR test asserts the solver and thread form that ran
(mmba_debug_band_solve's parts_used: -2 PCR in 512-thread workgroups, -3 in
256-thread ones; abi.PATH_PCR_WIDE = 0 pins the latter).  Unpinned, a grid of
at most 256 workgroups is resident in the 512-thread form on the 256 CUs of an
MI355X; a larger one takes whichever form the residency admits.

The alternative pivot chains (abi.PATH_PCR_CHAIN 1, 2) are held to the same
bar (CHAIN_MARGIN): at these condition numbers they stayed within 0.6 of the
floor, so no margin was raised.  A chain's margin may never exceed
far / (1000 floor) of any case (test_case_is_admissible).

What a purely arithmetic error at a deep level does here: with L_j scaled by
1 + 1e-6 from level 3 on in k_pcr_solve, test_gpu_band.py's 55 solves still
pass, and every PCR case of 17 blocks or more below fails with an error of
1e-6 .. 2e-4 (1e4 .. 1e6 bars).

Not covered: k_pcr_rhs_mc (the separator form's interior solve) has no hook;
the fall-back from PCR to BCR on a late granule is not provoked.

Measured on an MI355X (every run prints these figures with -s).  e64: the plain
fp64 solve's error; x: the device's; x/e64; x and the Newton term yn over their
floors max(e64, n eps) -- the bar is 1000 on both.  "512=256": the two thread
forms gave the same figures.  The 258-block system ran in the 256-thread form
(its grid of 264 is not resident in the 512-thread one).

   nb  w nG  solver                    e64        x   x/e64  x/floor yn/floor
    8  6  0  PCR default 512=256   3.1e-16  1.9e-15     6.1      1.1     0.81
   16  6  0  PCR default 512=256   7.0e-16  4.7e-15     6.7      1.3      1.3
   24  6  0  PCR default 512=256   2.5e-15  5.6e-15     2.2        1     0.88
   75  6  0  PCR default 512=256   4.4e-15  2.7e-14     6.1      1.6      1.5
  136  6  0  PCR default 512=256   4.6e-15  7.9e-14      17      2.6        2
  520  6  0  PCR default 512=256   1.2e-13  9.1e-13     7.6      7.7      5.8
    7  3  0  PCR default 512=256   5.7e-16  2.0e-15     3.5      1.3        1
   72  8  0  PCR default 512=256   2.2e-15  6.9e-15     3.1     0.43     0.59
   48 12  0  PCR default 512=256   1.0e-15  1.2e-14      12      1.1      1.1
  149 12  0  PCR default 512=256   3.6e-15  4.3e-14      12      1.3      1.1
  528 12  0  PCR default 512=256   3.0e-15  3.0e-13   1e+02      2.6        2
  149  9  0  PCR default 512=256   1.9e-15  4.6e-14      24      1.4      1.1
  272 16  0  PCR default 512=256   3.3e-15  9.4e-14      28      1.6      1.4
   24 23  0  PCR default 512=256   7.7e-16  6.2e-15     8.1      1.2      1.1
   48 23  0  PCR default 512=256   1.2e-15  8.1e-15     6.8     0.76     0.74
  221 23  0  PCR default 512=256   5.4e-15  1.2e-14     2.2     0.25     0.38
  792 23  0  PCR default 512=256   1.0e-14  3.4e-13      34        2      1.8
  221 17  0  PCR default 512=256   1.8e-14  6.5e-14     3.6      1.3      1.3
  408 24  0  PCR default 512=256   1.1e-14  2.9e-14     2.6     0.32     0.89
 2056  6  0  PCR default 512=256   2.5e-13  7.8e-12      31       17       13
 6173 23  0  PCR default 256       2.8e-13  5.6e-12      20      4.1      2.9
   75  6  0  PCR chain 0 512=256   4.4e-15  2.7e-14     6.1      1.6      1.5
   75  6  0  PCR chain 1 512=256   4.4e-15  9.9e-15     2.3     0.59     0.49
   75  6  0  PCR chain 2 512=256   4.4e-15  7.4e-15     1.7     0.44      0.4
  149 12  0  PCR chain 0 512=256   3.6e-15  4.3e-14      12      1.3      1.1
  149 12  0  PCR chain 1 512=256   3.6e-15  2.4e-14     6.7     0.72     0.54
  149 12  0  PCR chain 2 512=256   3.6e-15  6.6e-15     1.8      0.2    0.098
  221 23  0  PCR chain 0 512=256   5.4e-15  1.2e-14     2.2     0.25     0.38
  221 23  0  PCR chain 1 512=256   5.4e-15  2.7e-14       5     0.54     0.49
  221 23  0  PCR chain 2 512=256   5.4e-15  2.0e-14     3.7     0.41     0.38
 1000 23  5  BCR                   6.2e-14  3.4e-13     5.5      1.5      1.4
 1000 32 16  BCR                   2.0e-14  1.2e-13       6     0.53     0.39
  300  6 32  BCR                   1.8e-14  2.9e-13      16      3.9        3
  500 16 17  BCR                   3.0e-14  1.2e-13       4        1      0.9
 1560 24 24  BCR                   8.6e-14  9.0e-14       1     0.26     0.25
  300  6 48  BCR                   1.9e-14  3.1e-13      16        4        3
 1000 23 40  BCR                   6.8e-15  2.5e-13      37      1.1     0.77
  520  6  0  BCR (P = -2)          1.2e-13  9.6e-13       8      8.1      6.5
  528 12  0  BCR (P = -2)          3.0e-15  3.0e-13   1e+02      2.5        2
  792 23  0  BCR (P = -2)          1.0e-14  3.4e-13      34        2      1.8
  792 23  0  band P = 1            1.0e-14  2.6e-13      26      1.5      1.3
  792 23  0  band P = 3            1.0e-14  2.6e-13      26      1.5      1.4
 1000 23  5  band P = 6            6.2e-14  2.7e-13     4.4      1.2      1.1
 1000 40 16  band P = 4            4.9e-15  2.5e-13      51      1.1        1
  640 60  3  band P = 1            1.3e-14  9.9e-14     7.6     0.69     0.69
 1000 40 48  band P = 1            1.7e-14  3.0e-13      18      1.3      1.3
"""
import functools

import numpy as np
import pytest

from mayamatchmovesolver_amd import abi

EPS = 2.0 ** -52
MU = 1e-6
MARGIN = 1000.0        # x max(e64, n eps): test_gpu_damped_step.py's STEP_MARGIN
CAP = 1e-7             # a bar above this: the case is not admissible (STEP_CAP)
FAR_OVER_BAR = 1000.0  # a cut level stands this far above the bar
ASYM = 0.01            # max|L_j - L_j^T| of every first sub-diagonal block
# margin of each pivot chain over max(e64, n eps)
CHAIN_MARGIN = {0: MARGIN, 1: MARGIN, 2: MARGIN}


def block_size(w):
    return max(8, (w + 7) // 8 * 8)


def chain_band_spd(nb, w, nG, mu=MU, seed=0):
    rng = np.random.default_rng(seed)
    n = nb + nG
    F = np.zeros((n, n))
    for i in range(nb):
        k = min(w, i)
        F[i, i] = 1.0
        if k:
            a = rng.uniform(0.1, 1.0, k)
            F[i, i - k:i] = -a / a.sum()
    if nG:
        F[nb:, :nb] = rng.uniform(-1, 1, (nG, nb)) * 0.3 / np.sqrt(max(nb, 1))
        F[nb:, nb:] = np.tril(rng.uniform(-1, 1, (nG, nG)) * 0.3) + np.eye(nG)
    S = F @ F.T
    d = 1.0 / np.sqrt(np.diag(S))
    S = S * d[:, None] * d[None, :]
    S = 0.5 * (S + S.T)
    S[np.arange(n), np.arange(n)] = 1.0 + mu
    return S


def residual_extended(S, nb, w, R, X):
    """R - S X in numpy.longdouble, in row blocks over the columns of the band
    and the arrow (S is zero elsewhere)."""
    n = S.shape[0]
    out = R.astype(np.longdouble)
    for r0 in range(0, nb, 256):
        r1 = min(nb, r0 + 256)
        cols = np.r_[max(0, r0 - w):min(nb, r1 + w), nb:n]
        out[r0:r1] -= S[r0:r1][:, cols].astype(np.longdouble) @ X[cols]
    if n > nb:
        out[nb:] -= S[nb:].astype(np.longdouble) @ X
    return out


class Case:
    """One system: S, its right-hand sides, the reference and the bars."""

    def __init__(self, nb, w, nG, S=None):
        assert np.finfo(np.longdouble).eps < 1e-18, "numpy.longdouble is not extended precision"
        self.nb, self.w, self.nG, self.n = nb, w, nG, nb + nG
        self.K = block_size(w)
        self.nblk = (nb + self.K - 1) // self.K
        self.S = chain_band_spd(nb, w, nG, seed=nb * 31 + w * 7 + nG) if S is None else S
        n, K = self.n, self.K
        rng = np.random.default_rng(nb + 5)
        R = np.zeros((n, 6))
        R[:, :4] = rng.standard_normal((n, 4))
        self.first = slice(0, min(K, nb))
        self.last = slice((self.nblk - 1) * K, nb)
        R[self.first, 4] = 1.0
        R[self.last, 5] = 1.0
        self.R = R
        x64 = np.linalg.solve(self.S, R)
        Sinv = np.linalg.inv(self.S)  # one factorisation for the refinement's solves
        X = x64.astype(np.longdouble)
        for _ in range(4):
            X = X + (Sinv @ residual_extended(self.S, nb, w, R, X).astype(np.float64))
        self.x_ref = X
        xmax = np.max(np.abs(X), axis=0)
        self.e64 = float(np.max(np.max(np.abs(x64 - X), axis=0) / xmax))
        self.floor = max(self.e64, n * EPS)
        self.bar = MARGIN * self.floor
        self.y_ref = np.sum(R.astype(np.longdouble) * X, axis=0)
        y64 = np.sum(R * x64, axis=0)
        self.ey64 = float(np.max(np.abs(y64 - self.y_ref) / np.abs(self.y_ref)))
        self.bar_y = MARGIN * max(self.ey64, n * EPS)
        if self.nblk >= 2:
            self.far = float(min(np.max(np.abs(X[self.last, 4])) / xmax[4],
                                 np.max(np.abs(X[self.first, 5])) / xmax[5]))
        else:
            self.far = None

    def errors(self, solve):
        """(largest solution error, largest Newton-term error, parts_used) of a
        debug_band_solve closure over the case's right-hand sides."""
        ex = ey = 0.0
        used = set()
        for k in range(self.R.shape[1]):
            x, yn, u = solve(self.R[:, k])
            xr = self.x_ref[:, k]
            ex = max(ex, float(np.max(np.abs(x - xr)) / np.max(np.abs(xr))))
            ey = max(ey, float(abs(yn - self.y_ref[k]) / abs(self.y_ref[k])))
            used.add(u)
        assert len(used) == 1, used
        return ex, ey, used.pop()


@functools.lru_cache(maxsize=None)
def case(nb, w, nG):
    return Case(nb, w, nG)


# ---- the cases ----

# PCR (P = -1, no arrow): the smallest shapes at which each index path exists
PCR_SHAPES = [
    # K = 8
    (8, 6), (16, 6), (24, 6), (75, 6), (136, 6), (520, 6), (7, 3), (72, 8),
    # K = 16
    (48, 12), (149, 12), (528, 12), (149, 9), (272, 16),
    # K = 24
    (24, 23), (48, 23), (221, 23), (792, 23), (221, 17), (408, 24),
]
PCR_NINE_LEVELS = (2056, 6)    # 257 blocks, both forms
PCR_LARGEST = (6173, 23)       # 258 blocks, unpinned
# every chain x form on one ragged multi-level shape per K
PCR_CROSS = [(75, 6), (149, 12), (221, 23)]
BCR_ARROW = [(1000, 23, 5), (1000, 32, 16), (300, 6, 32), (500, 16, 17), (24 * 65, 24, 24),
             (300, 6, 48), (1000, 23, 40)]
BCR_ONLY = [(520, 6, 0), (528, 12, 0), (792, 23, 0)]
BAND = [(792, 23, 0, 1), (792, 23, 0, 3), (1000, 23, 5, 6), (1000, 40, 16, 4), (640, 60, 3, 1),
        (1000, 40, 48, 1)]
ALL_SYSTEMS = sorted({(nb, w, 0) for nb, w in PCR_SHAPES + [PCR_NINE_LEVELS, PCR_LARGEST]} |
                     set(BCR_ARROW) | set(BCR_ONLY) | {c[:3] for c in BAND})


# ---- CPU: every case is admissible ----

@pytest.mark.parametrize("nb,w,nG", ALL_SYSTEMS)
def test_case_is_admissible(nb, w, nG):
    c = case(nb, w, nG)
    S, K = c.S, c.K
    assert np.array_equal(S, S.T)
    i, j = np.indices((nb, nb), sparse=True)
    band = S[:nb, :nb]
    assert not np.any(band[np.abs(i - j) > w])
    if nb > w:
        assert np.all(np.diagonal(band, -w) != 0.0)  # half bandwidth exactly w
    for jb in range(1, c.nblk):
        L = np.zeros((K, K))
        rows = band[jb * K:(jb + 1) * K, (jb - 1) * K:jb * K]
        L[:rows.shape[0]] = rows
        assert np.max(np.abs(L - L.T)) >= ASYM, jb
    print("%5d %2d %2d  blocks %3d  e64 %.1e  bar %.1e  bar_y %.1e  far %s" %
          (nb, w, nG, c.nblk, c.e64, c.bar, c.bar_y, "-" if c.far is None else "%.1e" % c.far))
    assert c.bar <= CAP and c.bar_y <= CAP
    if c.nblk >= 2:
        assert c.far >= FAR_OVER_BAR * c.bar
        for m in CHAIN_MARGIN.values():
            assert m * c.floor <= c.far / FAR_OVER_BAR


def test_dominant_generator_has_no_far_field():
    """Why chain_band_spd exists: on test_gpu_band.py's diagonally dominant
    matrices the last of 65 blocks does not see the first at any bar."""
    from test_gpu_band import band_arrow_spd
    c = Case(520, 6, 0, S=band_arrow_spd(520, 6, 0, seed=0))
    assert c.bar <= CAP
    assert c.far < FAR_OVER_BAR * c.bar
    assert c.far < 1e-100


# ---- GPU ----

FORMS = {"wide": -2, "narrow": -3}


def run(gpu_ctx, c, P, label):
    from mayamatchmovesolver_amd.solver import debug_band_solve
    ex, ey, used = c.errors(debug_band_solve(gpu_ctx, c.S, c.nb, c.w, c.nG, P))
    print("%5d %2d %2d %-14s used %2d  e64 %.1e  x %.1e (%.2g e64, %.2g floor)  "
          "yn %.1e (%.2g floor)" % (c.nb, c.w, c.nG, label, used, c.e64, ex, ex / c.e64,
                                    ex / c.floor, ey, ey / max(c.ey64, c.n * EPS)))
    return ex, ey, used


def pcr_check(gpu_ctx, paths, nb, w, form, chain=None):
    c = case(nb, w, 0)
    if form == "narrow":
        paths(abi.PATH_PCR_WIDE, 0)
    if chain is not None:
        paths(abi.PATH_PCR_CHAIN, chain)
    margin = CHAIN_MARGIN[chain or 0]
    ex, ey, used = run(gpu_ctx, c, -1, "pcr c%s %s" % ("-" if chain is None else chain, form))
    if form == "narrow" or 8 * ((c.nblk + 7) // 8) <= 256:
        assert used == FORMS[form]
    else:
        assert used in (-2, -3)
    assert ex <= margin * c.floor
    assert ey <= margin * max(c.ey64, c.n * EPS)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["wide", "narrow"])
@pytest.mark.parametrize("nb,w", PCR_SHAPES + [PCR_NINE_LEVELS])
def test_pcr_coupled(nb, w, form, gpu_ctx, paths):
    pcr_check(gpu_ctx, paths, nb, w, form)


@pytest.mark.gpu
def test_pcr_coupled_largest(gpu_ctx, paths):
    pcr_check(gpu_ctx, paths, *PCR_LARGEST, "wide")


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["wide", "narrow"])
@pytest.mark.parametrize("chain", [0, 1, 2])
@pytest.mark.parametrize("nb,w", PCR_CROSS)
def test_pcr_coupled_chains(nb, w, chain, form, gpu_ctx, paths):
    pcr_check(gpu_ctx, paths, nb, w, form, chain)


@pytest.mark.gpu
@pytest.mark.parametrize("nb,w,nG,P", [c + (-1,) for c in BCR_ARROW] +
                         [c + (-2,) for c in BCR_ONLY] + BAND)
def test_bcr_and_band_coupled(nb, w, nG, P, gpu_ctx):
    c = case(nb, w, nG)
    ex, ey, used = run(gpu_ctx, c, P, "P %d" % P)
    assert used not in (-2, -3)
    if P > 1:
        assert used > 1
    assert ex <= c.bar
    assert ey <= c.bar_y
