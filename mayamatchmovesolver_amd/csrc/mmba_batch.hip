// mmba_batch.hip -- per-frame solve mode as ONE launch: the plain
// instantiations of k_batch_lm (mmba_batch_dev.h: one workgroup per frame runs
// that frame's whole MINPACK solve) and the dispatch.  The object form's
// instantiations are made in mmba_batch_obj.hip, and only there.
#include "mmba_batch_dev.h"

namespace mmba {

void launch_batch_lm(hipStream_t s, const DevProblem &P, const BatchArgs &B, int nf_max,
                     const BatchObjDev *O) {
    if (B.nf <= 0) return;
    if (O) {  // some frame's block holds an object-frame parameter
        launch_batch_lm_obj(s, P, B, nf_max, *O);
        return;
    }
    if (nf_max <= 8)
        k_batch_lm<8, 8><<<B.nf, BT, 0, s>>>(P, B, NoObjRec());
    else if (nf_max <= 16)
        k_batch_lm<16, PCMAX><<<B.nf, BT, 0, s>>>(P, B, NoObjRec());
    else
        k_batch_lm<32, PCMAX><<<B.nf, BT, 0, s>>>(P, B, NoObjRec());
}

}  // namespace mmba
