// mm_passk_k4.hip -- instances of the K-step kernel (mm_passk.hpp) for K = 4.
#include "mm_passk.hpp"

namespace mm {

const KernelInst* passk_inst_k4(const InstKey& q) {
    switch (q.na) {
        case 1: return passk_inst<4, 1, false>(q);
        default: return nullptr;
    }
}

}  // namespace mm
