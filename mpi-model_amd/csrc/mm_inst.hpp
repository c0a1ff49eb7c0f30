// mm_inst.hpp -- one descriptor per kernel instance (host side). A unit that builds kernel
// instances exports one lookup from a typed key to the instance's descriptor; launching and
// the occupancy estimate work on the descriptor, so an instance is named in one place and
// the planner sizes segments for exactly the kernel that runs. Not part of the public
// boundary.
#pragma once

#include <algorithm>

#include "mm_internal.hpp"

namespace mm {

struct KernelInst {
    const void* fn;  // the kernel's address (by-value PassArgs as its only argument)
    int threads;     // per workgroup
};

// The descriptor of kernel Kern (an instance of a __global__ template), one per instance.
template <auto Kern, int Threads>
const KernelInst* inst_of() {
    static const KernelInst inst{reinterpret_cast<const void*>(Kern), Threads};
    return &inst;
}

// Enqueue `blocks` workgroups of the instance on `s`; the status is this launch's, not an
// earlier call's.
inline hipError_t launch_inst(const KernelInst& k, long long blocks, const PassArgs& a,
                              hipStream_t s) {
    void* argv[] = {const_cast<PassArgs*>(&a)};
    (void)hipGetLastError();
    (void)hipLaunchKernel(k.fn, dim3((unsigned)blocks), dim3((unsigned)k.threads), argv, 0, s);
    return hipGetLastError();
}

// Resident workgroups per CU of an instance, from its register count and its static LDS:
// gfx950 gives each SIMD lane 512 registers (VGPRs and AGPRs together, allocated in granules
// of 8), at most 8 waves per SIMD, 4 SIMDs and 160 KiB of LDS per CU (MI355X_MICROARCH.md).
// The runtime's occupancy query is not used: after `import torch` it answers for these
// kernels with half the true occupancy (profiles/r02/occupancy_probe.log), which would
// halve the waves of every plan. 0 if the kernel cannot be queried.
inline int inst_blocks_per_cu(const KernelInst& k) {
    hipFuncAttributes fa;
    if (hipFuncGetAttributes(&fa, k.fn) != hipSuccess) {
        (void)hipGetLastError();  // a failed query must not surface at the next launch
        return 0;
    }
    const int regs = (fa.numRegs + 7) / 8 * 8;
    const int waves_per_simd = regs > 0 ? std::min(8, 512 / regs) : 8;
    int blocks = waves_per_simd * 4 / (k.threads / 64);
    if (fa.sharedSizeBytes > 0) blocks = std::min(blocks, (int)(160 * 1024 / fa.sharedSizeBytes));
    return blocks;
}

// What selects an instance of the K-step kernels.
// mm_passk_kernel, mm_wide_kernel, mm_fieldk_kernel, mm_closedk_kernel
enum InstFamily { kInstPassK, kInstWide, kInstFieldK, kInstClosedK };
struct InstKey {
    InstFamily family;
    int k;     // fused steps per pass
    int cols;  // columns per lane
    int na;    // attributes
    bool seg;  // segment schedule; false: border blocks of kBorderRows rows (mm_passk_kernel)
    bool red;  // every level's sums into the partials
    bool nt;   // non-temporal stores (segment schedule; the four-attribute K = 8 wide
               // instances store non-temporal whatever this says: only those are built)
    // mm_wide_kernel with four attributes:
    bool ring;  // the pre-chain is the ring t -> t+1 mod 4, no post-chain, every attribute
                // diffuses (K = 8: the compile-time-chain instance)
    bool post;  // the pass has a post-chain (K = 8: the instance that runs one)
    int nd;     // K = 8: the pass's attributes 0..nd-1 diffuse, the others do not (the engine
                // relabels them so; the instance has nd at compile time)
};

// The lookups, one per instance unit: the descriptor of the instance the key selects, or
// nullptr for a key the unit does not build. Each is the only place that maps the key's
// run-time values to its unit's template arguments.
using InstLookup = const KernelInst* (*)(const InstKey&);
#define MM_INST_DECL(name) const KernelInst* name(const InstKey& q);
// mm_passk_k<K>.hip: na = 1 for K 1..10, na 2..4 for K 1..2
MM_INST_DECL(passk_inst_k1) MM_INST_DECL(passk_inst_k2) MM_INST_DECL(passk_inst_k3)
MM_INST_DECL(passk_inst_k4) MM_INST_DECL(passk_inst_k5) MM_INST_DECL(passk_inst_k6)
MM_INST_DECL(passk_inst_k7) MM_INST_DECL(passk_inst_k8) MM_INST_DECL(passk_inst_k9)
MM_INST_DECL(passk_inst_k10)
// mm_wide_k<K>.hip: one attribute, 4 columns per lane (K = 20: one object per sums x
// non-temporal instance, and the unit that tries the four)
MM_INST_DECL(wide_inst_k4) MM_INST_DECL(wide_inst_k8) MM_INST_DECL(wide_inst_k12)
MM_INST_DECL(wide_inst_k16) MM_INST_DECL(wide_inst_k20)
MM_INST_DECL(wide_inst_k20_r0_n0) MM_INST_DECL(wide_inst_k20_r0_n1)
MM_INST_DECL(wide_inst_k20_r1_n0) MM_INST_DECL(wide_inst_k20_r1_n1)
MM_INST_DECL(wide_inst_k16_r0_n0) MM_INST_DECL(wide_inst_k16_r0_n1)  // K = 16: the same
MM_INST_DECL(wide_inst_k16_r1_n0) MM_INST_DECL(wide_inst_k16_r1_n1)
// mm_wide6_k20.hip: the fused K = 20 pass, cols = kWide6Cols (mm_wide6_kernel; one instance:
// non-temporal stores, no sums)
MM_INST_DECL(wide6_inst_k20)
// four attributes, 2 columns per lane. mm_widea_k4.hip: any pass of K = 4;
// mm_widear_k8.hip: the ring instance; mm_widea_k8.hip, one object per instance: nd = N
// diffusing attributes with (P = 1) or without (P = 0) a post-chain
MM_INST_DECL(widea_inst_k4) MM_INST_DECL(widear_inst_k8)
MM_INST_DECL(widea8_inst_n1_p0) MM_INST_DECL(widea8_inst_n1_p1)
MM_INST_DECL(widea8_inst_n2_p0) MM_INST_DECL(widea8_inst_n2_p1)
MM_INST_DECL(widea8_inst_n3_p0) MM_INST_DECL(widea8_inst_n3_p1)
MM_INST_DECL(widea8_inst_n4_p0) MM_INST_DECL(widea8_inst_n4_p1)
// mm_fieldk_k<K>.hip: the K-step rate-field kernel, one attribute, K = 2..kFieldMaxSteps
MM_INST_DECL(fieldk_inst_k2) MM_INST_DECL(fieldk_inst_k3) MM_INST_DECL(fieldk_inst_k4)
// mm_closedk_k<K>.hip: the K-step closed rate-field kernel, one attribute, K =
// 2..kClosedMaxSteps
MM_INST_DECL(closedk_inst_k2) MM_INST_DECL(closedk_inst_k3) MM_INST_DECL(closedk_inst_k4)
#undef MM_INST_DECL

// The instance of a key among all units (mm_kernels_k.hip), nullptr if none builds it.
const KernelInst* find_inst(const InstKey& q);
// K fused steps of a one-pass flow program on the instance of `q` (mm_kernels_k.hip).
// mm_passk_kernel (NA = 1: K 1..10, one diffusion; NA 2..4: K 1..2, diffusions and transfer
// chains): a.seg: segment schedule, a.th / a.th_edge rows per wave; else 4-row blocks (a.th
// = kBorderRows); a.nstrips = ceil(W / passk_out_cols(k)); sums into partials[wave][k][na].
// mm_wide_kernel: one workgroup of wide_waves_per_block(k, c, na, ring) waves per strip
// segment, segment schedule only (a.seg; a.th / a.th_edge rows per block, a.waves_a /
// a.waves_total count BLOCKS), a.nstrips = ceil(W / wide_out_cols(k, c)); sums into
// partials[block][k][na].
// mm_fieldk_kernel (one attribute, one rate-field diffusion, K 2..kFieldMaxSteps): a.seg:
// segment schedule; else 4-row border blocks (a.th = kBorderRows); a.field[0] the rate field;
// strips, row ranges, waves and partials as mm_passk_kernel's.
// mm_closedk_kernel (one attribute, one closed rate-field diffusion, K 2..kClosedMaxSteps):
// a.seg: segment schedule; else 4-row border blocks (a.th = kBorderRows); a.field[0] the rate
// field; a.nstrips = ceil(W / closedk_out_cols(k)); row ranges, waves and partials as
// mm_passk_kernel's.
// hipErrorInvalidValue for a key no unit builds.
hipError_t launch_kstep(const InstKey& q, const PassArgs& a, hipStream_t s);

}  // namespace mm
