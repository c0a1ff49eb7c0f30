// mm_kernels_k.hip -- the K-step kernels' one table of instances (templates: mm_passk.hpp,
// mm_wide.hpp, mm_fieldk.hpp and mm_closedk.hpp; instance units with their lookups:
// mm_passk_k1..10.hip, mm_wide*.hip, mm_fieldk_k2..4.hip, mm_closedk_k2..4.hip),
// their launch, and the fixed-order level-sum finalize kernel.
#include "mm_wide.hpp"

namespace mm {

namespace {

// Fixed-order sums of the levels in `mask` of partials[n][k][na] -> one history entry of
// na sums per level, slots from the device counter (graph-replayable). One workgroup per
// (level of the mask, attribute), all in parallel: workgroup b sums level j = the e-th set
// bit of mask (e = b / na) of attribute a = b % na -- each thread a strided run of the n
// partials, then a tree over the 256 threads (the order of the single-workgroup kernel
// this replaces, which walked the K x NA sums one after another: 37.8 us per C5 pass,
// profiles/r03/r3q). Partials slot a holds attribute (perm >> 2a) & 3 (the engine's
// relabelled passes). Every workgroup reads the slot counter hist_n[0]; the last one to
// finish (hist_n[1] counts them, agent-scope atomics: the workgroups run on every XCD)
// advances it and resets the count for the next launch.
__global__ __launch_bounds__(256) void mm_level_sums_kernel(const double* partials, long long n,
                                                            int k, int na, int mask,
                                                            double* hist,
                                                            unsigned long long* hist_n,
                                                            long long cap, int perm) {
    __shared__ double red[256];
    const int e = (int)blockIdx.x / na, a = (int)blockIdx.x % na;
    int j = 0;
    for (int c = -1; j < k; ++j)
        if (((mask >> j) & 1) && ++c == e) break;
    double s = 0.0;
    for (long long i = threadIdx.x; i < n; i += 256) s = s + partials[(i * k + j) * na + a];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
        if ((int)threadIdx.x < m) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const unsigned long long slot =
            __hip_atomic_load(hist_n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const long long idx = (long long)slot + e;
        if (idx < cap) hist[idx * na + ((perm >> (2 * a)) & 3)] = red[0];
        // the slot is read before this workgroup counts itself done (acq_rel orders them)
        const unsigned long long done = __hip_atomic_fetch_add(
            hist_n + 1, 1ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (done == (unsigned long long)gridDim.x - 1) {
            const int entries = __builtin_popcount((unsigned)mask);
            __hip_atomic_store(hist_n, slot + (unsigned long long)entries, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(hist_n + 1, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

}  // namespace

hipError_t launch_finalize_levels(const double* partials, long long n, int k, int na, int mask,
                                  double* hist, unsigned long long* hist_n, long long cap,
                                  hipStream_t s, int perm) {
    const int entries = __builtin_popcount((unsigned)mask);
    if (entries == 0) return hipSuccess;
    hipLaunchKernelGGL(mm_level_sums_kernel, dim3((unsigned)(entries * na)), dim3(256), 0, s,
                       partials, n, k, na, mask, hist, hist_n, cap, perm);
    return hipGetLastError();
}

static_assert(seg_prefetch<1>() == kSegPrefetch1,
              "mm_geom.hpp: passk_max_rows counts MM_SEG_U1 rows");

// Every instance unit's lookup; each answers for its own keys alone.
const KernelInst* find_inst(const InstKey& q) {
    static constexpr InstLookup kUnits[] = {
        passk_inst_k1,     passk_inst_k2,     passk_inst_k3,     passk_inst_k4,
        passk_inst_k5,     passk_inst_k6,     passk_inst_k7,     passk_inst_k8,
        passk_inst_k9,     passk_inst_k10,    wide_inst_k4,      wide_inst_k8,
        wide_inst_k12,     wide_inst_k16,     wide_inst_k20,     wide6_inst_k20,
        widea_inst_k4,
        widear_inst_k8,    widea8_inst_n1_p0, widea8_inst_n1_p1, widea8_inst_n2_p0,
        widea8_inst_n2_p1, widea8_inst_n3_p0, widea8_inst_n3_p1, widea8_inst_n4_p0,
        widea8_inst_n4_p1, fieldk_inst_k2,    fieldk_inst_k3,    fieldk_inst_k4,
        closedk_inst_k2,   closedk_inst_k3,   closedk_inst_k4};
    for (InstLookup unit : kUnits)
        if (const KernelInst* inst = unit(q)) return inst;
    return nullptr;
}

// A pass of no work is not launched -- unless waves_a < 0 marks it as mm_prepare's
// priming dispatch: one workgroup that leaves at its first instruction (waves_total = 0),
// which loads the kernel and sizes the queue's scratch for it ahead of the run.
hipError_t launch_kstep(const InstKey& q, const PassArgs& a, hipStream_t s) {
    if (a.waves_total <= 0 && a.waves_a >= 0) return hipSuccess;
    const KernelInst* inst = find_inst(q);
    if (!inst) return hipErrorInvalidValue;
    // at least one workgroup: a dispatch with no work (mm_prepare) still reaches the queue
    long long blocks = std::max<long long>(a.waves_total, 1);  // mm_wide_kernel: one per segment
    if (q.family == kInstFieldK) {
        if (!a.field[0] || a.field_mask != 1) return hipErrorInvalidValue;
        if (!q.seg && a.th != kBorderRows) return hipErrorInvalidValue;
        blocks = std::max<long long>(1, (a.waves_total + kWavesPerBlock - 1) / kWavesPerBlock);
    } else if (q.family == kInstClosedK) {
        if (!a.field[0] || a.field_mask != 1) return hipErrorInvalidValue;
        if (!q.seg && a.th != kBorderRows) return hipErrorInvalidValue;
        blocks = std::max<long long>(1, (a.waves_total + kWavesPerBlock - 1) / kWavesPerBlock);
    } else if (q.family == kInstPassK) {
        if (!q.seg && a.th != kBorderRows) return hipErrorInvalidValue;
        blocks = std::max<long long>(1, (a.waves_total + kWavesPerBlock - 1) / kWavesPerBlock);
        if (a.xcd_remap) blocks = (blocks + 7) / 8 * 8;
    }
    return launch_inst(*inst, blocks, a, s);
}

}  // namespace mm
