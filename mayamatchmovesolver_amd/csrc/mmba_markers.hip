// mmba_markers.hip -- refresh of the measurements of a built plan
// (mmba_plan_set_marker_values): marker positions and weights change between
// two solves of one structure far more often than the structure does, and on
// the device they are three arrays in device observation order
// (DevProblem::obs_xy, obs_sqrtw and, with the rolling shutter, obs_tau).
//
// The caller's arrays go through a page-locked staging mirror into a device
// staging block in the caller's order, one copy per array given; one launch
// then permutes them into device order through the plan's ref_of_dev and the
// x,y source of every device observation recorded at build (B4: an
// observation of a remapped MMSG plan borrows the position of another marker
// at its frame).  No sort, map or structure pass runs: the host validates,
// packs and takes the square roots of the weights -- std::sqrt, the function
// Plan::build calls, so a refreshed plan holds the bits of a fresh one for
// every input, not only for those a test happens to draw.
//
// One thread per device observation; each array is written by consecutive
// threads at consecutive addresses (x,y as one 16-byte store), plain vector
// stores, no atomics, no LDS.
#include <cmath>
#include <cstring>

#include "mmba_kernels.h"
#include "mmba_plan.h"

namespace mmba {

// xy_src (nullable: every observation reads its own obs_xy entry): >= 0 an
// index into obs_xy, < 0 the index -(src + 1) into mkr_frame_xy.  A NULL
// staging array leaves what it would set as it is.  obs_tau (rolling shutter)
// follows obs_xy's own y (the expression of Plan::build; the B4 remap and the
// rolling shutter exclude each other).
__global__ void k_marker_set(int M, const int *__restrict__ ref_of_dev,
                             const int *__restrict__ xy_src, const double *__restrict__ xy,
                             const double *__restrict__ fxy, const double *__restrict__ sqrtw,
                             const double *__restrict__ obs_rs, double *__restrict__ obs_xy,
                             double *__restrict__ obs_sqrtw, double *__restrict__ obs_tau) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const int r = ref_of_dev[i];
    const int src = xy_src ? xy_src[i] : r;
    const double *from = src >= 0 ? xy : fxy;
    if (from) {
        const size_t at = src >= 0 ? (size_t)src : (size_t)(-(src + 1));
        reinterpret_cast<double2 *>(obs_xy)[i] = reinterpret_cast<const double2 *>(from)[at];
    }
    if (sqrtw) obs_sqrtw[i] = sqrtw[r];
    if (obs_tau && xy) obs_tau[i] = obs_rs[i] * (0.5 - xy[2 * (size_t)r + 1]);
}

void launch_marker_set(hipStream_t s, int M, const int *ref_of_dev, const int *xy_src,
                       const double *xy, const double *fxy, const double *sqrtw,
                       const double *obs_rs, double *obs_xy, double *obs_sqrtw, double *obs_tau) {
    if (M <= 0) return;
    k_marker_set<<<nblk(M, 256), 256, 0, s>>>(M, ref_of_dev, xy_src, xy, fxy, sqrtw, obs_rs,
                                              obs_xy, obs_sqrtw, obs_tau);
}

// The staging blocks, host and device alike: [obs_xy (2 Mg) | mkr_frame_xy
// (2 K F, only where the plan borrows from it) | sqrt(obs_weight) (Mg)] -- the
// two x,y lists first, so both start on a 16-byte boundary.
void Plan::setup_marker_refresh(int K) {
    mk_nfxy = mk_frame_src ? 2 * (size_t)K * F : 0;
    const size_t total = std::max<size_t>(3 * (size_t)Mg + mk_nfxy, 1);
    d_mk = dalloc<double>(total);
    MMBA_HIP(hipHostMalloc((void **)&h_mk, sizeof(double) * total, hipHostMallocDefault));
}

// The arrays are valid (mmba_plan_set_marker_values checks them before any
// plan is touched) and mkr_frame_xy is NULL unless the plan borrows from it.
void Plan::set_marker_values(const double *xy, const double *weight, const double *fxy) {
    const size_t nxy = 2 * (size_t)Mg;
    double *hx = h_mk, *hf = h_mk + nxy, *hw = hf + mk_nfxy;
    double *dx = d_mk, *df = d_mk + nxy, *dw = df + mk_nfxy;
    if (xy) {
        std::memcpy(hx, xy, sizeof(double) * nxy);
        MMBA_HIP(hipMemcpyAsync(dx, hx, sizeof(double) * nxy, hipMemcpyHostToDevice, s));
    }
    if (fxy) {
        std::memcpy(hf, fxy, sizeof(double) * mk_nfxy);
        MMBA_HIP(hipMemcpyAsync(df, hf, sizeof(double) * mk_nfxy, hipMemcpyHostToDevice, s));
    }
    if (weight) {
        for (int r = 0; r < Mg; ++r) hw[r] = std::sqrt(weight[r]);
        MMBA_HIP(hipMemcpyAsync(dw, hw, sizeof(double) * Mg, hipMemcpyHostToDevice, s));
    }
    launch_marker_set(s, M, d_ref_of_dev, d_xy_src, xy ? dx : nullptr, fxy ? df : nullptr,
                      weight ? dw : nullptr, d_obs_rs, d_obs_xy, d_obs_sqrtw,
                      rs_on ? d_obs_tau : nullptr);
    MMBA_HIP(hipGetLastError());
    host_sync();  // the staging mirror is free for the next call
    // Nothing a previous entry point left behind describes these measurements:
    // the outputs in d_f / d_eu / d_ed (mmba_plan_outputs, and the d_ed that
    // mmba_plan_error_metrics reduces), a deferred epilogue reduction, a
    // Jacobian enqueued ahead of a decision, the staged slots (InFlight), and
    // the parameter and record passes later calls would skip.
    outputs_ready = false;
    fl.reset();
    params_at = nullptr;
    recs_full_at = nullptr;
}

}  // namespace mmba
