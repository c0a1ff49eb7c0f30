// mm_wide_k16.hip -- instances of the level-split K-step kernel (mm_wide.hpp) for K = 16:
// 4 level(s) per wave, 4 waves per workgroup.
// Tuning (tools/libsweep.py, profiles/r03/sweep_w16): 2 input rows prefetched by the first
// wave (243 VGPRs, no spill; 4 rows: 256 VGPRs with a spill) -- 1.5 % faster at 32768^2.
#ifndef MM_WIDE_U
#define MM_WIDE_U 2
#endif
#include "mm_wide.hpp"

// One object per instance (sums or not x non-temporal stores or not), as mm_wide_k20.hip:
// the Makefile builds this unit with MM_PART_RED / MM_PART_NT set for each of the four
// instances (they compile in parallel; in one object the unit was the build's longest job
// by far), and once without them for the dispatcher below.
#define MM_CAT4(a, b, c, d) a##b##c##d
#define MM_PN(f, r, n) MM_CAT4(f, r, _n, n)

namespace mm {

#if defined(MM_PART_RED) && defined(MM_PART_NT)

const KernelInst* MM_PN(wide_inst_k16_r, MM_PART_RED, MM_PART_NT)(const InstKey& q) {
    if (!wide_key<4, 1, 4, 4>(q) || q.red != (MM_PART_RED != 0) || q.nt != (MM_PART_NT != 0))
        return nullptr;
    return wide_inst_v<4, 1, 4, 4, MM_WIDE_MIN_WAVES, MM_PART_RED != 0, MM_PART_NT>();
}

#else

const KernelInst* wide_inst_k16(const InstKey& q) {
    for (InstLookup part : {wide_inst_k16_r0_n0, wide_inst_k16_r0_n1, wide_inst_k16_r1_n0,
                            wide_inst_k16_r1_n1})
        if (const KernelInst* i = part(q)) return i;
    return nullptr;
}

#endif

}  // namespace mm
