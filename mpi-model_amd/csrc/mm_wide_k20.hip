// mm_wide_k20.hip -- instances of the level-split K-step kernel (mm_wide.hpp) for K = 20:
// 5 level(s) per wave, 4 waves per workgroup.
// Tuning (tools/libsweep.py, profiles/r03/var_k20): levels in ascending order (no pend
// registers: VGPR spills 504 -> 27) and 2 input rows prefetched -- 7 % faster at 32768^2
// than the pend hand-off with 4 rows (8260 vs 8891 us per 20-step pass on one box).
#ifndef MM_WIDE_ASC
#define MM_WIDE_ASC 1
#endif
#ifndef MM_WIDE_U
#define MM_WIDE_U 2
#endif
#ifndef MM_K20_KW
#define MM_K20_KW 5  // levels per wave (20 / MM_K20_KW waves per workgroup)
#endif
#include "mm_wide.hpp"

// One object per instance (sums or not x non-temporal stores or not): the Makefile builds
// this unit with MM_PART_RED / MM_PART_NT set for each of the four instances (they compile
// in parallel), and once without them for the dispatcher below.
#define MM_K20_P (20 / MM_K20_KW)
#define MM_CAT4(a, b, c, d) a##b##c##d
#define MM_PN(f, r, n) MM_CAT4(f, r, _n, n)

namespace mm {

#if defined(MM_PART_RED) && defined(MM_PART_NT)

const KernelInst* MM_PN(wide_inst_k20_r, MM_PART_RED, MM_PART_NT)(const InstKey& q) {
    if (!wide_key<4, 1, MM_K20_KW, MM_K20_P>(q) || q.red != (MM_PART_RED != 0) ||
        q.nt != (MM_PART_NT != 0))
        return nullptr;
    return wide_inst_v<4, 1, MM_K20_KW, MM_K20_P, MM_WIDE_MIN_WAVES, MM_PART_RED != 0,
                       MM_PART_NT>();
}

#else

const KernelInst* wide_inst_k20(const InstKey& q) {
    for (InstLookup part : {wide_inst_k20_r0_n0, wide_inst_k20_r0_n1, wide_inst_k20_r1_n0,
                            wide_inst_k20_r1_n1})
        if (const KernelInst* i = part(q)) return i;
    return nullptr;
}

static_assert(MM_K20_P == kWide20Waves, "mm_geom.hpp: waves per workgroup of the K = 20 instance");

#endif

}  // namespace mm
