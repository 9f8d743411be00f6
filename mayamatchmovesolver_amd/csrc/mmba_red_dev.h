// The row reduction of k_reduce_multi as a device function: every launch
// that reduces a partial row in its own extra workgroups uses this one, so
// the slots get the same bits whichever launch carries them.
#pragma once
#include <hip/hip_runtime.h>

#include "mmba_kernels.h"
#include "mmba_wave_dev.h"

namespace mmba {

// One partial row reduced by one 256-thread workgroup: thread t combines
// entries t, t + 256, ... in that order, then block_tree.
template <bool SC1>
__device__ __forceinline__ double reduce_row_block(const double *partial, const RedRow &rw,
                                                   double *red) {
    const bool mx = rw.is_max != 0;
    double s = 0.;
    for (int i = threadIdx.x; i < rw.n; i += blockDim.x) {
        const double q = SC1 ? ld_sc1(&partial[rw.off + i]) : partial[rw.off + i];
        s = mx ? fmax(s, q) : s + q;
    }
    red[threadIdx.x] = s;
    __syncthreads();
    block_tree(red, mx);
    const double v = red[0];
    __syncthreads();
    return v;
}

}  // namespace mmba
