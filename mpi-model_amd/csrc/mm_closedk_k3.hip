// mm_closedk_k3.hip -- instances of the K-step closed rate-field kernel (mm_closedk.hpp) for K = 3.
#include "mm_closedk.hpp"

namespace mm {

const KernelInst* closedk_inst_k3(const InstKey& q) { return closedk_inst<3>(q); }

}  // namespace mm
