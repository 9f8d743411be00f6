// mmba_batch_obj.hip -- the object form of the batched per-frame solve: the
// OBJ instantiations of k_batch_lm (mmba_batch_dev.h), in this translation
// unit only.  Per-frame object tracking -- the camera locked, the object's
// bundles surveyed, its six pose curves solved frame by frame -- runs every
// frame's solve in one launch; each workgroup builds its frame's object
// records in LDS (world_matrix once per slot) and the FD columns of the
// object-frame parameters move the bundle, not the camera.  Compiled beside
// the plain instantiations the transform-chain code would move their register
// allocation (they sit at 256 VGPRs), as mmba_object.hip's does for
// k_jacobian.
#include "mmba_batch_dev.h"

namespace mmba {

void launch_batch_lm_obj(hipStream_t s, const DevProblem &P, const BatchArgs &B, int nf_max,
                         const BatchObjDev &O) {
    if (B.nf <= 0) return;
    if (nf_max <= 8)
        k_batch_lm<8, 8, true><<<B.nf, BT, 0, s>>>(P, B, O);
    else if (nf_max <= 16)
        k_batch_lm<16, PCMAX, true><<<B.nf, BT, 0, s>>>(P, B, O);
    else
        k_batch_lm<32, PCMAX, true><<<B.nf, BT, 0, s>>>(P, B, O);
}

}  // namespace mmba
