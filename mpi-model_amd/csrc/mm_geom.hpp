// mm_geom.hpp -- the kernels' geometry as plain arithmetic: constants and per-instance
// shapes that both the kernel units (through mm_internal.hpp) and the host-only planner
// (mm_plan.cpp) need. No HIP include; a unit whose tuning macro fixes one of these values
// static_asserts that it agrees.
#pragma once

namespace mm {

constexpr int kMaxAttr = 4;     // SoA attributes per fused pass (config C5: 4)
constexpr int kMaxChain = 4;    // elementwise transfers before / after a pass's diffusion
                                // (a longer chain starts a new pass; 4 holds config C5's
                                // chain and, against 8, frees kernel-argument SGPRs: C5 -8 %)
constexpr int kStripCols = 128; // columns per wave: 64 lanes x double2 (16 B per lane)
constexpr int kWavesPerBlock = 4;
constexpr int kBlock = 64 * kWavesPerBlock;
constexpr int kMaxSteps = 10;    // fused steps per pass of mm_passk_kernel (one attribute)
constexpr int kMaxWide = 20;     // fused steps per pass of mm_wide_kernel (one attribute)
constexpr int kGhost = kMaxWide;  // ghost rows above and below a slab (K fused steps need K)
constexpr int kBorderRows = 4;     // rows per wave of the K-step kernel's border launches
constexpr int kSegPrefetch1 = 8;   // mm_passk.hpp seg_prefetch<1>() (MM_SEG_U1)
constexpr int kWide20Waves = 4;    // waves per workgroup, K = 20 (mm_wide_k20.hip: 20 / MM_K20_KW)
constexpr int kWideRingWaves = 4;  // the ring instance (mm_widear_k8.hip: 8 / MM_WIDEAR_KW)
constexpr int kWide6Cols = 6;      // columns per lane of mm_wide6_kernel's interior strips (K = 20)

// 1 + (i > 0) + (i < n-1) inside [0, n), 0 outside: cnt = span(x)*span(y) - 1 (constexpr:
// the kernels and the engine's host code share it)
constexpr int span3(long long n, long long i) {
    return (i >= 0 && i < n) ? 1 + (i > 0) + (i < n - 1) : 0;
}

inline int passk_out_cols(int k) { return kStripCols - 4 * ((k + 1) / 2); }

inline int passk_max_steps(int na) { return na == 1 ? kMaxSteps : 2; }

// largest segment (rows) whose buffer offsets stay below 2^31 at this pitch
inline long long passk_max_rows(int k, long long pitch) {
    // every buffer offset of a wave (rows x pitch x 8 B, plus the OOB marker) stays < 2^31
    return (1LL << 31) / (pitch * 8) - (3 * k + 2 * kSegPrefetch1 + 8);
}

// mm_fieldk_kernel (mm_fieldk.hpp): fused steps per rate-field pass, K = 2..kFieldMaxSteps
// (include/mpimodel.h MM_FIELD_MAX_STEPS); its strips are mm_passk_kernel's (passk_out_cols).
constexpr int kFieldMaxSteps = 4;
constexpr int kFieldPrefetch = 8;  // rows of v in flight per wave
// Rows of the rate field a wave holds in registers: kFieldPrefetch rows ahead of level 1
// and the 2(K-1) rows behind it that the later levels still multiply by, rounded up to a
// multiple of the prefetch depth (the steady loop is unrolled once around the ring).
constexpr int field_ring(int k) {
    return (kFieldPrefetch + 2 * (k - 1) + kFieldPrefetch - 1) / kFieldPrefetch * kFieldPrefetch;
}

// largest segment (rows) of a K-step rate-field pass: every offset into the state and into
// the field buffer (a ring ahead of the rows, and the segment rounded up to a whole ring)
// stays below 2^31
inline long long fieldk_max_rows(int k, long long pitch) {
    return (1LL << 31) / (pitch * 8) - (3 * k + 2 * field_ring(k) + 8);
}

// mm_closedk_kernel (mm_closedk.hpp): fused steps per closed rate-field pass, K =
// 2..kClosedMaxSteps (include/mpimodel.h MM_CLOSED_MAX_STEPS).
constexpr int kClosedMaxSteps = 4;
// Output columns of its strips. A strip that loads columns [c0, c0 + 128) knows the count of
// open neighbours only of columns c0+1 .. c0+126, so its level-K values are valid from column
// c0 + K + 1 on: the discarded halo is floor((K + 2) / 2) lanes, at least K + 1 columns, a side.
constexpr int closedk_halo_cols(int k) { return 2 * ((k + 2) / 2); }
constexpr int closedk_out_cols(int k) { return kStripCols - 2 * closedk_halo_cols(k); }
// Rows of the rate field a wave holds in registers: as field_ring, and the row that runs
// ahead of level 1 (a row's count needs the openness of the row below it).
constexpr int closed_ring(int k) {
    return (kFieldPrefetch + 2 * (k - 1) + 1 + kFieldPrefetch - 1) / kFieldPrefetch * kFieldPrefetch;
}
// largest segment (rows) of a K-step closed pass: as fieldk_max_rows, with the rate field one
// row further ahead
inline long long closedk_max_rows(int k, long long pitch) {
    return (1LL << 31) / (pitch * 8) - (3 * k + 2 * closed_ring(k) + 9);
}

inline bool wide_has(int k, int c, int na) {
    if (na > 1) return na == 4 && c == 2 && (k == 4 || k == 8);
    return c == 4 && (k == 4 || k == 8 || k == 12 || k == 16 || k == 20);
}

inline int wide_out_cols(int k, int c) {
    return 64 * c - 2 * c * ((k + c - 1) / c);  // 64 lanes less ceil(K / C) halo lanes a side
}

// Column tiling of the fused six-column K = 20 pass (mm_wide6_kernel): the frame's first strip
// [0, col) at 4 columns per lane, `strips` strips of wide_out_cols(20, 6) columns from col on at
// 6 columns per lane, and rstrips strips at 4 columns per lane over [rcol, W). The six-column
// strips run the FAST body alone, so every column they load (one halo, 24 columns, past their
// output columns) is an interior column of the grid: the right part keeps at least 25 columns,
// the grid's last column among them. strips == 0: W too narrow.
struct Wide6Cols {
    int col, rcol, strips, rstrips;
};
inline Wide6Cols wide6_cols(long long W) {
    const int o4 = wide_out_cols(kMaxWide, 4), o6 = wide_out_cols(kMaxWide, kWide6Cols);
    const int halo = kWide6Cols * ((kMaxWide + kWide6Cols - 1) / kWide6Cols);
    const long long room = W - o4 - (halo + 1);
    const int n = room >= o6 && W < (1LL << 30) ? (int)(room / o6) : 0;
    const int rcol = o4 + n * o6;
    return {o4, rcol, n, n ? (int)((W - rcol + o4 - 1) / o4) : 0};
}

inline int wide_waves_per_block(int k, int c, int na, bool ring) {
    if (!wide_has(k, c, na)) return 0;
    if (na > 1 && k == 8 && ring) return kWideRingWaves;
    if (na == 1 && k == 20) return kWide20Waves;
    // one attribute: K / 4 levels per wave, 4 level groups; four attributes: mm_widea_k4
    // 1 level per wave, mm_widea_k8 2
    return 4;
}

}  // namespace mm
