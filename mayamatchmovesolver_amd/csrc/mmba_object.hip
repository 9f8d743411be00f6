// mmba_object.hip -- object records: the world matrices of moving bundle
// parents, once per evaluation.
//
// A rigid object is a transform keyed per frame with its bundles parented
// under it.  bundle_position walks the parent chain for every observation,
// and the FD Jacobian walks it again for every column that moves the bundle
// (a sincos triple and a 4x4 product per level, in one thread's serial fp64
// stream).  All observations of one (parent, frame) share that matrix, and
// all their rows share the matrix of each column's perturbed point.
//
// Plan::build lists one record set per (bundle-parent transform whose chain
// holds an animated or solved attribute, frame with observations): a base
// slot and one variant slot per parameter that moves the parent at that frame
// (camera-frame block parameters -- VF_OBJ -- and bundle-side globals alike).
// k_obj_records builds every slot with world_matrix and the slot's Override,
// one thread per slot; k_jacobian / k_residual (their OREC instantiations)
// then form W (tx, ty, tz, 1) per observation and column (orec_position,
// mmba_geom.h) -- the arithmetic bundle_position applies to the same matrix.
// Those instantiations of the templates in mmba_obs_dev.h are made here, and
// only here (launch_residual_orec, launch_residual_jp_orec,
// launch_jacobian_orec): compiled into mmba_kernels.hip they move the register
// allocation of that file's other k_jacobian instantiations.
// It runs with every records launch (launch_records), so the records follow
// the attribute block wherever the camera records do: the Jacobian's point,
// the trial point, the first evaluation after mmba_plan_set_attr_values.
#include <hip/hip_runtime.h>

#include "mmba_obs_dev.h"

namespace mmba {

// 64-thread workgroups like k_records (short latency-bound chains); the
// logical block order is XCD-contiguous, as the sets are numbered in the
// observations' camera-frame order and the residual passes read them so.
__global__ void __launch_bounds__(64) k_obj_records(DevProblem P, ObjRecDev O,
                                                    const double *__restrict__ ext_pert,
                                                    int base_only) {
    const int slot = xcd_remap(blockIdx.x, gridDim.x) * 64 + threadIdx.x;
    if (slot >= O.n) return;
    const int p = O.par[slot];
    if (p >= 0 && base_only) return;
    const int set = O.set[slot];
    Override ov{-1, 0.};
    if (p >= 0) {
        ov.attr = P.p_attr[p];
        ov.value = ext_pert[p];
    }
    double W[16];
    world_matrix(P, O.tf[2 * set], O.tf[2 * set + 1], ov, W);
    double *rec = &O.rec[(size_t)slot * ORECSZ];
#pragma unroll
    for (int k = 0; k < ORECSZ; ++k) rec[k] = W[k];
}

void launch_obj_records(hipStream_t s, const DevProblem &P, const ObjRecDev &O,
                        const double *ext_pert, int base_only) {
    if (O.n <= 0) return;
    k_obj_records<<<(O.n + 63) / 64, 64, 0, s>>>(P, O, ext_pert, base_only);
}


// The record-reading instantiations of k_residual / k_jacobian
// (mmba_obs_dev.h), in this translation unit only.

void launch_residual_orec(hipStream_t s, const DevProblem &P, const ObjRecDev &O,
                          const double *recs, double *f, double *eu, double *ed, double *partial,
                          double *out, unsigned int *ticket, double *dist) {
    k_residual<false, false, false, true><<<nblk(P.M, 256), 256, 0, s>>>(
        P, recs, f, eu, ed, partial, out, ticket, nullptr, nullptr, nullptr, nullptr, nullptr, dist,
        O);
}

void launch_residual_jp_orec(hipStream_t s, const DevProblem &P, const ObjRecDev &O,
                             const double *recs, double *f, double *eu, double *ed,
                             double *partial, const double *J, const int *jcol, const int *nloc,
                             const double *pstep, double *partial_jp, double *dist) {
    k_residual<true, false, false, true><<<nblk(P.M, 256), 256, 0, s>>>(
        P, recs, f, eu, ed, partial, nullptr, nullptr, J, jcol, nloc, pstep, partial_jp, dist, O);
}

void launch_jacobian_orec(hipStream_t s, const DevProblem &P, const ObjRecDev &O,
                          const double *recs, const double *ext_pert, const double *step,
                          int solver_type, double *J, int *jcol, int *nloc,
                          const int *stale_param, double *eu, double *ed) {
    if (P.lens_uniform == MMBA_LENS_3DE_CLASSIC)
        k_jacobian<false, MMBA_LENS_3DE_CLASSIC, true><<<nblk(P.M, 128), 128, 0, s>>>(
            P, recs, ext_pert, step, solver_type, J, jcol, nloc, stale_param, eu, ed, CentralB(), O);
    else
        k_jacobian<false, -1, true><<<nblk(P.M, 128), 128, 0, s>>>(
            P, recs, ext_pert, step, solver_type, J, jcol, nloc, stale_param, eu, ed, CentralB(), O);
}

}  // namespace mmba
