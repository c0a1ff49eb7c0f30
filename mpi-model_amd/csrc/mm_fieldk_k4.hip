// mm_fieldk_k4.hip -- instances of the K-step rate-field kernel (mm_fieldk.hpp) for K = 4.
#include "mm_fieldk.hpp"

namespace mm {

const KernelInst* fieldk_inst_k4(const InstKey& q) { return fieldk_inst<4>(q); }

}  // namespace mm
