// mm_fieldk_k3.hip -- instances of the K-step rate-field kernel (mm_fieldk.hpp) for K = 3.
#include "mm_fieldk.hpp"

namespace mm {

const KernelInst* fieldk_inst_k3(const InstKey& q) { return fieldk_inst<3>(q); }

}  // namespace mm
