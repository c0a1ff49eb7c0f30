// mm_passk_k1.hip -- instances of the K-step kernel (mm_passk.hpp) for K = 1.
// Tuning (tools/libsweep.py --program c5, profiles/r02/libsweep_c5.log): the 3- and
// 4-attribute instances fit two waves per SIMD (<= 256 registers) with one row of the
// attributes prefetched; at the default 2 rows the 4-attribute K = 2 instance needs 257
// registers, one wave per SIMD, and runs 1.7x slower.
#ifndef MM_PASSK_MIN_WAVES
#define MM_PASSK_MIN_WAVES 2
#endif
#ifndef MM_SEG_UN
#define MM_SEG_UN 1
#endif
#include "mm_passk.hpp"

namespace mm {

const KernelInst* passk_inst_k1(const InstKey& q) {
    switch (q.na) {
        case 1: return passk_inst<1, 1, false>(q);
        case 2: return passk_inst<1, 2, true>(q);
        case 3: return passk_inst<1, 3, true>(q);
        case 4: return passk_inst<1, 4, true>(q);
        default: return nullptr;
    }
}

}  // namespace mm
