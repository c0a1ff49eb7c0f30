// mm_internal.hpp -- shared between the gfx950 kernels (mm_kernels.hip, mm_field.hip,
// mm_closed.hip, mm_kernels_k.hip) and the engine / C ABI (mm_engine.hip). The K-step kernels' instances
// and their launch: mm_inst.hpp. Not part of the public boundary.
#pragma once

#include <hip/hip_runtime.h>

#include "mm_geom.hpp"  // the constants and the kernels' geometry (hip-free)

namespace mm {

// One fused Jacobi pass over a row slab. Every buffer pointer points at owned row 0;
// rows -kGhost..-1 and h..h+kGhost-1 are ghost rows; local row r is global x_init+r.
//   u  = pre-chain transfers applied to the loaded cell values
//   per diffusing attribute a: out = rate_a*u, s = out/cnt, w = (u - out) + nb(s)
//   w  = post-chain transfers applied to w;  store w
// Rows [ra0, ra1) and [rb0, rb1) (local, half-open) are computed; the second
// range lets one launch cover both border rows of a halo-split step.
struct PassArgs {
    const double* in[kMaxAttr];
    double* out[kMaxAttr];
    long long H, W, x_init, pitch;
    int ra0, ra1, rb0, rb1;
    int th;                 // rows per wave
    int nstrips;            // column strips of 128 per row
    long long waves_a;      // waves covering range a
    long long waves_total;  // waves covering both ranges
    int diffuse_mask;       // bit a: attribute a diffuses in this pass
    int npre, npost;
    double drate[kMaxAttr];
    signed char pre_a[kMaxChain], pre_b[kMaxChain];
    signed char post_a[kMaxChain], post_b[kMaxChain];
    double pre_r[kMaxChain], post_r[kMaxChain];
    double* partials;       // REDUCE: [partial_base + wave][NA] (mm_passk_kernel: [..][K])
    long long partial_base;
    int xcd_remap;          // mm_passk_kernel: XCD-contiguous block order (grid padded to 8)
    int seg;                // mm_passk_kernel: segment schedule (th / th_edge rows per wave)
    int th_edge;            // mm_passk_kernel segments: rows per wave of the two edge strips
    const double* field[kMaxAttr];  // mm_field_kernel: rate field of attribute a (row 0, same
                                    // pitch and ghost rows as the attribute buffers)
    int field_mask;         // bit a: attribute a diffuses by field[a] in this pass
    // mm_wide6_kernel (mm_plan.hpp Wide6): rows [ra0, ra1), nstrips strips of the whole width
    int c6_top, c6_bot;     // interior rows [c6_top, c6_bot) between the two row bands
    int c6_col, c6_rcol;    // first output column of the six-column strips / of the strips
                            // right of them
    int c6_strips, c6_rstrips;  // six-column strips, strips right of them
    int c6_th;              // rows per interior segment (th: per frame segment between the bands)
    long long c6_band0, c6_band1, c6_frame;  // blocks before the end of the top band, of the
                                             // bottom band, of the frame (then the interior's)
};

// Launchers (mm_kernels.hip). All enqueue on `s` and return the launch status.
hipError_t launch_pass(int na, bool reduce, const PassArgs& a, hipStream_t s, int variant);
// One step of a rate-field pass (mm_field_kernel, mm_field.hip): the attributes of
// a.field_mask diffuse by their per-cell rate a.field[], the others are copied through. Row
// ranges, wave mapping and partials as launch_pass; a.th 8, or 1 (border rows). variant bit
// 0: non-temporal stores (one attribute).
hipError_t launch_field(int na, bool reduce, const PassArgs& a, hipStream_t s, int variant);
// One step of a closed rate-field pass (mm_closed_kernel, mm_closed.hip): the one attribute of
// a.field_mask diffuses by a.field[] among the cells whose rate is not zero, walls keep their
// bits, the other attributes are copied through. Arguments as launch_field.
hipError_t launch_closed(int na, bool reduce, const PassArgs& a, hipStream_t s, int variant);
// Append the levels of `mask` (bit j: step j of a K-step pass) of partials[n][k][na],
// each summed in a fixed order, to the history (na sums per entry).
// perm: partials slot i holds attribute (perm >> 2i) & 3 (relabelled passes).
hipError_t launch_finalize_levels(const double* partials, long long n, int k, int na, int mask,
                                  double* hist, unsigned long long* hist_n, long long cap,
                                  hipStream_t s, int perm);
hipError_t launch_fill(double* buf, long long pitch, long long H, long long W, long long x_init,
                       long long h, int mode, double value, unsigned long long seed, hipStream_t s);
hipError_t launch_point(double* buf, long long pitch, long long H, long long W, long long x_init,
                        long long h, long long sx, long long sy, double captured, double rate,
                        hipStream_t s);
// Sum partials[n][na] in a fixed order into hist[k][na], k = (*hist_n)++ (device
// counter, so the launch is graph-replayable); entries beyond cap are dropped.
hipError_t launch_finalize(const double* partials, long long n, int na, double* hist,
                           unsigned long long* hist_n, long long cap, hipStream_t s,
                           int entries = 1);
// Per-attribute sum of the owned rows of one buffer (no pass), into out[0].
hipError_t launch_slab_sum(const double* buf, long long pitch, long long W, long long h,
                           double* partials, long long nblocks, double* out_sum, hipStream_t s);

}  // namespace mm
