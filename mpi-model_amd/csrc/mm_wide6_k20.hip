// mm_wide6_k20.hip -- the fused K = 20 pass of large unsplit slabs (mm_wide.hpp
// mm_wide6_kernel): the frame at 4 columns per lane on mm_wide_k20.hip's code, the interior
// at 6 columns per lane on the FAST body alone. One instance: non-temporal stores, no sums
// (the only one a slab of the auto rule's size selects); same tuning as mm_wide_k20.hip.
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

#define MM_K20_P (20 / MM_K20_KW)

namespace mm {

const KernelInst* wide6_inst_k20(const InstKey& q) {
    // (non-temporal stores whatever q.nt says: a small grid forced here by MM_WIDE_COLS=6
    // stores the same values)
    if (q.family != kInstWide || q.k != 20 || q.cols != kWide6Cols || q.na != 1 || !q.seg || q.red)
        return nullptr;
    return inst_of<mm_wide6_kernel<4, kWide6Cols, MM_K20_KW, MM_K20_P, MM_WIDE_MIN_WAVES,
                                   MM_WIDE_U, MM_WIDE_B, 1>,
                   64 * MM_K20_P>();
}

static_assert(MM_K20_P == kWide20Waves, "mm_geom.hpp: waves per workgroup of the K = 20 instance");

}  // namespace mm
