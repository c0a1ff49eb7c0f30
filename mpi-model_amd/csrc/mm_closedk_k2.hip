// mm_closedk_k2.hip -- instances of the K-step closed rate-field kernel (mm_closedk.hpp) for K = 2.
#include "mm_closedk.hpp"

namespace mm {

const KernelInst* closedk_inst_k2(const InstKey& q) { return closedk_inst<2>(q); }

}  // namespace mm
