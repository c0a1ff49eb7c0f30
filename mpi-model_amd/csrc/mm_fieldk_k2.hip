// mm_fieldk_k2.hip -- instances of the K-step rate-field kernel (mm_fieldk.hpp) for K = 2.
#include "mm_fieldk.hpp"

namespace mm {

const KernelInst* fieldk_inst_k2(const InstKey& q) { return fieldk_inst<2>(q); }

}  // namespace mm
