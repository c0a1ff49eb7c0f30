// mm_wide_k12.hip -- instances of the level-split K-step kernel (mm_wide.hpp) for K = 12:
// 3 level(s) per wave, 4 waves per workgroup.
#include "mm_wide.hpp"

namespace mm {

const KernelInst* wide_inst_k12(const InstKey& q) {
    return wide_inst<4, 1, 3, 4, MM_WIDE_MIN_WAVES>(q);
}

}  // namespace mm
