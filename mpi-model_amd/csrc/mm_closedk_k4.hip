// mm_closedk_k4.hip -- instances of the K-step closed rate-field kernel (mm_closedk.hpp) for K = 4.
#include "mm_closedk.hpp"

namespace mm {

const KernelInst* closedk_inst_k4(const InstKey& q) { return closedk_inst<4>(q); }

}  // namespace mm
