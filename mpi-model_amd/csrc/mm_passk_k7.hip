// mm_passk_k7.hip -- instances of the K-step kernel (mm_passk.hpp) for K = 7 (one attribute).
// Tuning (tools/libsweep.py, profiles/r02): two waves per SIMD (<= 256 VGPRs) and 6 rows
// prefetched per wave; with the register file's other half a second wave hides the
// K-level VALU chains.
#ifndef MM_PASSK_MIN_WAVES
#define MM_PASSK_MIN_WAVES 2
#endif
#ifndef MM_SEG_U1
#define MM_SEG_U1 6
#endif
#include "mm_passk.hpp"

namespace mm {

const KernelInst* passk_inst_k7(const InstKey& q) {
    switch (q.na) {
        case 1: return passk_inst<7, 1, false>(q);
        default: return nullptr;
    }
}

}  // namespace mm
