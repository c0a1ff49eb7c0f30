// mm_widea_k4.hip -- instances of the level-split K-step kernel (mm_wide.hpp) for K = 4
// and several attributes (config C5: four, with transfer chains): 2 columns per lane,
// 1 level per wave, 4 waves per workgroup, rows handed on in groups of 2 (the LDS ring
// of a group of 4 rows holds 96 KiB per workgroup). Pre- and post-chains with run-time
// operands (chain_asm: the first n slots of a chain run, a scalar branch inside the asm
// skips the rest; outflows leaving the system land on the pad pair).
#ifndef MM_WIDE_U
#define MM_WIDE_U 2
#endif
#ifndef MM_WIDE_B
#define MM_WIDE_B 2
#endif
#define MM_CHAIN_ASM 1
#define MM_CHAIN_POST 1
#include "mm_wide.hpp"

namespace mm {

// any four-attribute pass of K = 4, whatever its chains and diffusing attributes
const KernelInst* widea_inst_k4(const InstKey& q) { return wide_inst<2, 4, 1, 4, 2>(q); }

}  // namespace mm
