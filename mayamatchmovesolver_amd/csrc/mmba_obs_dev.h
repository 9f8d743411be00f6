// mmba_obs_dev.h -- the per-observation kernel templates k_residual and
// k_jacobian, with the helpers they need.  A header because two translation
// units instantiate them: mmba_kernels.hip every form from before object
// records, mmba_object.hip the record-reading forms (OREC).  Kept apart on
// purpose: with the OREC instantiations compiled in mmba_kernels.hip the
// register allocation of the other k_jacobian instantiations moved (classic
// forward 245 -> 253 VGPRs, generic forward 73 -> 99 spilled VGPRs).
#pragma once

#include <type_traits>

#include "mmba_geom.h"
#include "mmba_kernels.h"
#include "mmba_wave_dev.h"

namespace mmba {

// Frame-sharding ownership (all-true when unsharded).
MMBA_DEV bool own_obs(const DevProblem &P, int i) { return !P.obs_own || P.obs_own[i]; }
MMBA_DEV bool own_cf(const DevProblem &P, int cf) { return !P.cf_own || P.cf_own[cf]; }
MMBA_DEV bool own_bnd(const DevProblem &P, int b) { return !P.bnd_own || P.bnd_own[b]; }
MMBA_DEV bool own_mask(const int *m, int i) { return !m || m[i]; }

// Deterministic single-launch reduction epilogue (see the reductions section).
template <bool MAX>
__device__ __forceinline__ void finish_blocks(double v, double *partial, double *out,
                                              unsigned int *ticket, int blk = -1) {
    if (blk < 0) blk = blockIdx.x;
    __shared__ int last;
    __shared__ double red[256];
    if (threadIdx.x == 0) {
        if (!ticket) {
            partial[blk] = v;
        } else {
            __hip_atomic_store(&partial[blk], v, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
            __threadfence();  // release the partial before the ticket
            last = atomicAdd(ticket, 1u) == gridDim.x - 1;
        }
    }
    if (!ticket) return;
    __syncthreads();
    if (!last) return;
    __threadfence();  // acquire the other blocks' partials
    double a = 0.;
    for (int i = threadIdx.x; i < (int)gridDim.x; i += blockDim.x) {
        const double q = __hip_atomic_load(&partial[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        a = MAX ? fmax(a, q) : a + q;
    }
    red[threadIdx.x] = a;
    __syncthreads();
    block_tree(red, MAX);
    if (threadIdx.x == 0) {
        *out = red[0];
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// -------------------------------------------------------------------------
// Residuals (measureErrors).  Writes f (device order), user deviation and
// distance, and one partial sum of squares per block.
// -------------------------------------------------------------------------
// JP: the trial-point evaluation also forms (J p)_obs = sum_l J_l p[jcol_l]
// from the Jacobian blocks of the current x (lmder's ||J p|| for prered)
// into a second partial row.
// FAST: every bundle is fast and no camera has a lens (the transform-chain
// and lens code, and their registers, are compiled out).
// RS: rolling shutter (mmba_rs.hip): each observation's camera record is
// its own scanline pose (camera_record_rs), not the camera-frame's.
// OREC: object records (mmba_object.hip): a bundle under a moving parent
// takes the parent's world matrix from its record set instead of walking the
// transform chain.  The tables are a kernel argument of these instantiations
// only (an empty struct otherwise).
template <bool OREC>
using ObjArg = std::conditional_t<OREC, ObjRecDev, NoObjRec>;

template <bool JP, bool FAST, bool RS = false, bool OREC = false>
__global__ void __launch_bounds__(256) k_residual(DevProblem P, const double *__restrict__ recs,
                                                  double *f, double *eu, double *ed,
                                                  double *partial, double *out,
                                                  unsigned int *ticket,
                                                  const double *__restrict__ J,
                                                  const int *__restrict__ jcol,
                                                  const int *__restrict__ nloc,
                                                  const double *__restrict__ pstep,
                                                  double *partial_jp, double *dist,
                                                  ObjArg<OREC> O) {
    __shared__ double red[256];
    const int lb = xcd_remap(blockIdx.x, gridDim.x);  // logical block (XCD-contiguous)
    const int i = lb * blockDim.x + threadIdx.x;
    double s = 0., sj = 0.;
    if (i < P.M) {
        const int cf = P.obs_cf[i];
        const int b = P.obs_bnd[i];
        const int fr = P.obs_frame[i];
        const Override none{-1, 0.};
        double bp[3];
        if (FAST) {
            const double *br = &P.brec[(size_t)b * BREC];
            bp[0] = br[0];
            bp[1] = br[1];
            bp[2] = br[2];
        } else if constexpr (OREC) {
            const int oset = O.obs_set[i];
            if (oset >= 0) orec_position(P, O, b, fr, oset, -1, none, bp);
            else base_bundle(P, b, fr, bp);
        } else {
            base_bundle(P, b, fr, bp);
        }
        double lc[MMBA_LENS_NUM_ATTRS];
        int inst = -1;
        const int hl = FAST ? MMBA_LENS_NONE : obs_lens_inst(P, i, inst);
        if (hl) inst_coeffs(P, inst, none, lc);
        const double *rec = &recs[(size_t)P.cf_var_off[cf] * CAMREC];
        double rloc[RS ? CAMREC : 1];
        if constexpr (RS) {
            camera_record_rs(P, cf, P.obs_tau[i], -1, 0., rloc);
            rec = rloc;
        }
        Resid r = residual_l(P, rec, bp, P.obs_xy[2 * i], P.obs_xy[2 * i + 1], P.obs_sqrtw[i],
                             hl, lc);
        f[2 * i] = r.ex;
        f[2 * i + 1] = r.ey;
        if (eu) {
            eu[2 * i] = r.ux;
            eu[2 * i + 1] = r.uy;
            ed[i] = r.dist;
        }
        if (dist) dist[i] = r.dist;  // errorDistanceList of this point (RMS at the accepted x)
        if (own_obs(P, i)) {
            s = r.ex * r.ex + r.ey * r.ey;
            if constexpr (JP) {
                const int M = P.M;
                double ax = 0., ay = 0.;
                const int nl = nloc[i];
                if (P.jcol_implicit) {
                    // uniform plans: column l is camera variant l (l < nv), then
                    // the bundle's parameters (k_jacobian_u's order).  Eight
                    // columns' index, step and J loads issued before their
                    // products (the sums in column order as before)
                    const int voff = P.cf_var_off[cf];
                    const int nv = P.cf_var_off[cf + 1] - voff - 1;
                    const int4 p4 = P.bnd_p4[b];
                    for (int l0 = 0; l0 < nl; l0 += 8) {
                        double jx[8], jy[8], pv[8];
#pragma unroll
                        for (int k = 0; k < 8; ++k) {
                            const int l = l0 + k;
                            if (l < nl) {
                                const int a = l - nv;
                                const int p = l < nv ? P.cf_var_param[voff + 1 + l]
                                                     : (a == 0 ? p4.x : (a == 1 ? p4.y : p4.z));
                                pv[k] = pstep[p];
                                jx[k] = J[(size_t)(2 * l) * M + i];
                                jy[k] = J[(size_t)(2 * l + 1) * M + i];
                            }
                        }
#pragma unroll
                        for (int k = 0; k < 8; ++k) {
                            if (l0 + k < nl) {
                                ax += jx[k] * pv[k];
                                ay += jy[k] * pv[k];
                            }
                        }
                    }
                } else {
                    for (int l = 0; l < nl; ++l) {
                        const double pv = pstep[jcol[(size_t)l * M + i]];
                        ax += J[(size_t)(2 * l) * M + i] * pv;
                        ay += J[(size_t)(2 * l + 1) * M + i] * pv;
                    }
                }
                sj = ax * ax + ay * ay;
            }
        }
    }
    if constexpr (JP) {
        red[threadIdx.x] = sj;
        __syncthreads();
        // block_tree written out (as below): the call changes this kernel's
        // instructions (the operands of each add swap places)
        for (int w = 128; w > 0; w >>= 1) {
            if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x == 0) partial_jp[lb] = red[0];
        __syncthreads();
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    finish_blocks<false>(red[0], partial, out, ticket, lb);
}

// -------------------------------------------------------------------------
// FD Jacobian blocks per observation (K1/K2 in SURVEY 7): same differences
// as solveFunc_calculateJacobianMatrixForParameter, evaluated only for the
// parameters that can change this observation (all other entries of the
// reference column are exactly zero).
// -------------------------------------------------------------------------
// CEN: central differences / B15 compiled in (CB.recs != nullptr).  The
// forward-difference build drops the deltaB evaluations and is held to two
// waves per SIMD (256 VGPRs, some spilled; one wave at 340 registers before):
// C5 1.21 against 1.33 ms per solve (profiles/r5_jac/).
// OREC: object records (mmba_object.hip) compiled in: the position of a
// bundle under a moving parent is W (tx, ty, tz, 1) with W the record of the
// column's parameter (the base record where the parameter does not move the
// parent), not a walk of the transform chain per column.
template <bool OREC>
__device__ __forceinline__ void moved_bundle(const DevProblem &P, const ObjArg<OREC> &O, int b,
                                             int fr, int oset, int p, const Override &ov,
                                             double *bp) {
    if constexpr (OREC) {
        if (oset >= 0) {
            orec_position(P, O, b, fr, oset, p, ov, bp);
            return;
        }
    }
    bundle_position(P, b, fr, ov, bp);
}

template <bool CEN, int LT = -1, bool OREC = false>
__global__ void __launch_bounds__(128, CEN ? 1 : 2) k_jacobian(DevProblem P, const double *__restrict__ recs,
                                                  const double *__restrict__ ext_pert,
                                                  const double *__restrict__ step,
                                                  int solver_type, double *J, int *jcol,
                                                  int *nloc, const int *__restrict__ stale_param,
                                                  double *eu, double *ed, CentralB CB,
                                                  ObjArg<OREC> O) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.M) return;
    const int M = P.M;
    const int cf = P.obs_cf[i];
    const int b = P.obs_bnd[i];
    const int fr = P.obs_frame[i];
    const double mx = P.obs_xy[2 * i], my = P.obs_xy[2 * i + 1], sw = P.obs_sqrtw[i];
    const Override none{-1, 0.};
    const int4 p4 = P.bnd_p4[b];
    double bp0[3];
    [[maybe_unused]] int oset = -1;
    if constexpr (OREC) {
        oset = O.obs_set[i];
        if (oset >= 0) orec_position(P, O, b, fr, oset, -1, none, bp0);
        else base_bundle(P, b, fr, bp0);
    } else {
        base_bundle(P, b, fr, bp0);
    }
    double lc0[MMBA_LENS_NUM_ATTRS];
    int inst = -1;
    const int hl = obs_lens_inst(P, i, inst);
    if (hl) inst_coeffs(P, inst, none, lc0);
    const int voff = P.cf_var_off[cf];
    const int nvar = P.cf_var_off[cf + 1] - voff;
    const double *rec0 = &recs[(size_t)voff * CAMREC];
    const Resid r0 = residual_l<LT>(P, rec0, bp0, mx, my, sw, hl, lc0);
    const bool lmder = solver_type == MMBA_SOLVER_CMINPACK_LMDER;
    const int pstale = stale_param[fr];
    Resid rs = r0;
    int l = 0;
    double ljx = 0., ljy = 0.;  // last emitted column (bundle block record)
    // evalB: the column's second (deltaB) evaluation, run only for a central
    // column (CB.step[p] != 0)
    auto emit_s = [&](int p, const Resid &r, double st, auto &&evalB) {
        double jx, jy;
        const double sB = (CEN && lmder && CB.recs) ? CB.step[p] : 0.;
        if (sB != 0.) {  // central: (f(x + dA) - f(x + dB)) * 0.5 / (|dA| + |dB|)
            const Resid rb = evalB();
            jx = (r.ex - rb.ex) * sB;
            jy = (r.ey - rb.ey) * sB;
            if (p == pstale) rs = rb;  // the column's last measureErrors
        } else {
            if (lmder) {  // st = 1/delta, multiplied (adjust_solveFunc.cpp:395-402)
                jx = (r.ex - r0.ex) * st;
                jy = (r.ey - r0.ey) * st;
            } else {      // st = h, divided (fdjac2)
                jx = (r.ex - r0.ex) / st;
                jy = (r.ey - r0.ey) / st;
            }
            if (p == pstale) rs = r;
        }
        J[(size_t)(2 * l) * M + i] = jx;
        J[(size_t)(2 * l + 1) * M + i] = jy;
        jcol[(size_t)l * M + i] = p;
        ljx = jx;
        ljy = jy;
        ++l;
    };
    // camera-side parameters (variants 1..nvar-1)
    for (int v = 1; v < nvar && l < LMAX; ++v) {
        const int t = voff + v;
        const int p = P.cf_var_param[t];
        // (an object-frame parameter of the block, VF_OBJ, carries
        // VF_BUNDLE_SIDE too: its variant record repeats the base record's
        // doubles and its column moves the bundle; a bundle not under the
        // transform keeps its position: f - f = 0)
        const bool bside = (P.cf_var_flags[t] & VF_BUNDLE_SIDE) != 0;
        if (P.cf_var_flags[t] & VF_LENS) {
            // a lens coefficient in the camera-frame block: the lens loop's
            // column (below), at its place in the block -- where this
            // observation's lens instance holds the coefficient (B3 may give
            // it an instance another frame's parameter wrote: then f - f = 0)
            bool holds = false;
            if (hl)
                for (int q = P.inst_lpar_off[inst]; q < P.inst_lpar_off[inst + 1]; ++q)
                    holds |= P.inst_lpar[q] == p;
            double lc[MMBA_LENS_NUM_ATTRS];
            if (holds) inst_coeffs(P, inst, Override{P.p_attr[p], ext_pert[p]}, lc);
            emit_s(p, residual_l<LT>(P, rec0, bp0, mx, my, sw, hl, holds ? lc : lc0), step[p], [&]() {
                double lq[MMBA_LENS_NUM_ATTRS];
                if (holds) inst_coeffs(P, inst, Override{P.p_attr[p], CB.ext_pert[p]}, lq);
                return residual_l<LT>(P, rec0, bp0, mx, my, sw, hl, holds ? lq : lc0);
            });
            continue;
        }
        double bp[3] = {bp0[0], bp0[1], bp0[2]};
        if (bside) moved_bundle<OREC>(P, O, b, fr, oset, p, Override{P.p_attr[p], ext_pert[p]}, bp);
        emit_s(p, residual_l<LT>(P, &recs[(size_t)t * CAMREC], bp, mx, my, sw, hl, lc0), step[p],
               [&]() {
                   double bq[3] = {bp0[0], bp0[1], bp0[2]};
                   if (bside) bundle_position(P, b, fr, Override{P.p_attr[p], CB.ext_pert[p]}, bq);
                   return residual_l<LT>(P, &CB.recs[(size_t)t * CAMREC], bq, mx, my, sw, hl, lc0);
               });
    }
    if (CEN && CB.q15) {
        // B15 (Plan::b15): the camera-frame block's columns (the first pc
        // emitted) in the basis Q_cf (Q c = kappa e_0): J_s Q = J Q - f kappa
        // e_0^T with J the central differences of the block's own frame.  The
        // large f c part of the block lands in one column, so the block's
        // normal equations keep the accuracy of its differences.
        const int pc = P.cf_pc[cf];
        const double *Q = CB.q15 + (size_t)cf * PCMAX * PCMAX;
        const double kap = CB.kap15[cf];
        double ax[PCMAX], ay[PCMAX];
#pragma unroll
        for (int a = 0; a < PCMAX; ++a) {
            ax[a] = a < pc ? J[(size_t)(2 * a) * M + i] : 0.;
            ay[a] = a < pc ? J[(size_t)(2 * a + 1) * M + i] : 0.;
        }
#pragma unroll
        for (int a2 = 0; a2 < PCMAX; ++a2) {
            if (a2 >= pc) break;
            double sx = 0., sy = 0.;
#pragma unroll
            for (int a = 0; a < PCMAX; ++a) {
                sx = fma(ax[a], Q[a * PCMAX + a2], sx);
                sy = fma(ay[a], Q[a * PCMAX + a2], sy);
            }
            if (a2 == 0) {
                sx -= r0.ex * kap;
                sy -= r0.ey * kap;
            }
            J[(size_t)(2 * a2) * M + i] = sx;
            J[(size_t)(2 * a2 + 1) * M + i] = sy;
        }
    }
    // bundle-side parameters not already covered by a camera variant
    if (p4.w >= 0) {  // fast bundle: perturbed positions from the record
        const double *br = &P.brec[(size_t)b * BREC];
        double jb[8] = {0., 0., 0., 0., 0., 0., r0.ex, r0.ey};
        for (int a = 0; a < p4.w && l < LMAX; ++a) {
            const int p = a == 0 ? p4.x : (a == 1 ? p4.y : p4.z);
            const double bp[3] = {br[3 + 3 * a], br[4 + 3 * a], br[5 + 3 * a]};
            emit_s(p, residual_l<LT>(P, rec0, bp, mx, my, sw, hl, lc0), br[12 + a], [&]() {
                const double *bb = &CB.brec[(size_t)b * BREC];
                const double bq[3] = {bb[3 + 3 * a], bb[4 + 3 * a], bb[5 + 3 * a]};
                return residual_l<LT>(P, rec0, bq, mx, my, sw, hl, lc0);
            });
            jb[2 * a] = ljx;
            jb[2 * a + 1] = ljy;
        }
        // bundle block record, one 64-B record per observation (coalesced
        // store; k_ne_bnd_jb gathers one record per observation of a bundle
        // instead of 8 SoA rows): [jx_a, jy_a]_a, f_x, f_y
        if (P.JB) {
            double4 *dst = reinterpret_cast<double4 *>(&P.JB[(size_t)P.obs_bpos[i] * 8]);
            dst[0] = make_double4(jb[0], jb[1], jb[2], jb[3]);
            dst[1] = make_double4(jb[4], jb[5], jb[6], jb[7]);
        }
    }
    for (int q = p4.w >= 0 ? P.bnd_par_off[b + 1] : P.bnd_par_off[b];
         q < P.bnd_par_off[b + 1] && l < LMAX; ++q) {
        const int p = P.bnd_par[q];
        if (P.p_frame[p] >= 0 && P.p_frame[p] != fr) continue;
        if (P.p_both[p]) {
            bool seen = false;
            for (int v = 1; v < nvar; ++v) seen |= (P.cf_var_param[voff + v] == p);
            if (seen) continue;
        }
        double bp[3];
        moved_bundle<OREC>(P, O, b, fr, oset, p, Override{P.p_attr[p], ext_pert[p]}, bp);
        emit_s(p, residual_l<LT>(P, rec0, bp, mx, my, sw, hl, lc0), step[p], [&]() {
            double bq[3];
            bundle_position(P, b, fr, Override{P.p_attr[p], CB.ext_pert[p]}, bq);
            return residual_l<LT>(P, rec0, bq, mx, my, sw, hl, lc0);
        });
    }
    // the lens parameters this observation's lens instance holds (an
    // instance slot has one attribute, so overriding by attribute moves only
    // the slot the parameter writes)
    if (hl) {
        for (int q = P.inst_lpar_off[inst]; q < P.inst_lpar_off[inst + 1] && l < LMAX; ++q) {
            const int p = P.inst_lpar[q];
            // an animated parameter's column re-measures its own frame only
            // (adjust_solveFunc.cpp frameIndexEnable): the observations of
            // other frames that read the instance it writes keep f - f = 0
            if (P.p_frame[p] >= 0 && P.p_frame[p] != fr) continue;
            // a camera-frame block column (VF_LENS) of this row's own block;
            // another camera-frame's block hosts a coefficient several cameras
            // read (mmba_lens_shared.hip): a foreign row emits its column here
            if (P.p_class[p] == PC_CF && P.p_blk[p] == cf) continue;
            double lc[MMBA_LENS_NUM_ATTRS];
            inst_coeffs(P, inst, Override{P.p_attr[p], ext_pert[p]}, lc);
            emit_s(p, residual_l<LT>(P, rec0, bp0, mx, my, sw, hl, lc), step[p], [&]() {
                double lq[MMBA_LENS_NUM_ATTRS];
                inst_coeffs(P, inst, Override{P.p_attr[p], CB.ext_pert[p]}, lq);
                return residual_l<LT>(P, rec0, bp0, mx, my, sw, hl, lq);
            });
        }
    }
    nloc[i] = l;
    // errorList / errorDistanceList as left by the last FD column (Appendix B13).
    if (eu) {
        eu[2 * i] = rs.ux;
        eu[2 * i + 1] = rs.uy;
        ed[i] = rs.dist;
    }
}

}  // namespace mmba
