// mm_fieldk.hpp -- K fused steps of the rate-field diffusion (MM_FLOW_DIFFUSE_FIELD) per
// HBM pass, gfx950: temporal blocking of mm_field_kernel's step for a program that is one
// field diffusion of one attribute. A pass reads every cell's value and rate once, advances
// the value K steps in registers and writes it once: 24/K B per cell-update instead of 24 B.
// On a slab with a halo the interior rows run the segment schedule beside the exchange and
// the K border rows of each side the BLOCK schedule after it (fieldk_block below), which
// reads K ghost rows of the state and of the rate field (MM_FIELD_HALO, include/mpimodel.h).
//
// The schedule is mm_passk_kernel's SEGMENT schedule (mm_passk.hpp, header comment), whose
// strips, lane layout, wave map and descriptors it shares: a wave loads 128 columns (lane
// l: columns c0+2l, c0+2l+1 as one 16-B buffer load) and outputs the inner
// passk_out_cols(K); the +-1-column terms come from the adjacent lanes through DPP shifts,
// and the garbage that enters at the wave's edge lanes moves one column inward per level
// and stays in the discarded halo lanes. The wave slides down a segment of rows; level j
// keeps a three-row window in registers (the shares s of the row above and of the current
// row, d = v - out of the current row) and emits one row per input row. The levels are
// skewed: at iteration i level j consumes the row level j-1 emitted at iteration i-1 --
// input row i - 2(j-1) of the segment, whose first input row is rA - K -- so the K levels
// of an iteration are independent instruction streams. One rows_rsrc descriptor per wave
// and buffer: offsets past the range load 0 and drop stores, which is what keeps the rows
// outside the launch (the levels' fill, the iterations that round a segment up) harmless.
//
// The rate row. Every level multiplies by f of the row it consumes, 2(j-1) iterations
// after level 1 did. The rates stay in a register ring of field_ring(K) rows (mm_geom.hpp;
// 4 VGPRs per row and lane): a slot is loaded kFieldPrefetch or more iterations before
// level 1 reads it and reloaded as soon as level K has. The steady loop is unrolled once
// around the ring, so every slot index is a constant. (DESIGN.md 4.1 has the registers of
// each instance and what an LDS ring or a re-read per level would cost instead.)
//
// Arithmetic: each level is share_one / fprocess_row / femit_row of mm_field.hip, operation
// for operation (out = f*v by select, s = out*0.125 where cnt == 8, else the IEEE division,
// q = s(x-1) + s(x+1), t = q + s(x), nb = (t(y-1) + t(y+1)) + q, v' = (v - out) + nb; built
// with -ffp-contract=off), so K fused steps are bit-identical to K single steps. From level
// 1 on the kernel computes rows above row 0 and below row H-1, columns >= W and halo lanes;
// at every level those cells contribute s = 0 by select on the global row and column, never
// by multiplication (the pitch padding of v and f may hold NaN, and a cell beside the grid
// holds whatever the grid's edge cells sent it). The division runs only where a wave-uniform
// test says the row or the strip touches the grid's edge.
//
// This header holds the kernel template; mm_fieldk_k<K>.hip instantiate it (one translation
// unit per K) and mm_kernels_k.hip dispatches.
#pragma once

#include "mm_passk.hpp"

namespace mm {

namespace {

// One level's three-row window: the shares of the row above (sa) and of the current row
// (sm), the current row's d = v - out (dm), of this lane's two columns.
struct FWin {
    double sa0, sa1, sm0, sm1, dm0, dm1;
};

// Shares and d = v - out of this lane's two columns of row gx (mm_field.hip fprocess_row).
// FAST: the row has three in-grid rows and every loaded column two in-grid neighbours, so
// cnt == 8 throughout; else decided per row (wave-uniform), and a row or a column outside
// the grid (span 0) shares 0 by select whatever it holds.
template <bool FAST>
__device__ __forceinline__ void fk_share(const Lane& c, long long gx, double v0, double v1,
                                         double f0, double f1, double& s0, double& s1,
                                         double& d0, double& d1) {
    const int sx = FAST ? 3 : span3(c.H, gx);
    double out0, out1;
    if (FAST || (sx == 3 && c.fast_cols)) {
        out0 = f0 * v0;
        out1 = f1 * v1;
        s0 = out0 * 0.125;
        s1 = out1 * 0.125;
    } else {
        share_one(v0, f0, sx && c.sy0, sx * c.sy0 - 1, out0, s0);
        share_one(v1, f1, sx && c.sy1, sx * c.sy1 - 1, out1, s1);
    }
    d0 = v0 - out0;
    d1 = v1 - out1;
}

// Level input row m = 0 or 1: fill the window.
template <bool FAST>
__device__ __forceinline__ void fk_fill(const Lane& c, long long gx, int m, FWin& w, double v0,
                                        double v1, double f0, double f1) {
    double s0, s1, d0, d1;
    fk_share<FAST>(c, gx, v0, v1, f0, f1, s0, s1, d0, d1);
    if (m == 0) {
        w.sa0 = s0;
        w.sa1 = s1;
    } else {
        w.sm0 = s0;
        w.sm1 = s1;
        w.dm0 = d0;
        w.dm1 = d1;
    }
}

// Level input row m >= 2 (global row gx): emit the window's current row gx - 1
// (mm_field.hip femit_row) and slide the window.
template <bool FAST>
__device__ __forceinline__ void fk_emit(const Lane& c, long long gx, FWin& w, double v0, double v1,
                                        double f0, double f1, double& o0, double& o1) {
    double sn0, sn1, dn0, dn1;
    fk_share<FAST>(c, gx, v0, v1, f0, f1, sn0, sn1, dn0, dn1);
    const double q0 = w.sa0 + sn0, q1 = w.sa1 + sn1;
    const double t0 = q0 + w.sm0, t1 = q1 + w.sm1;
    const double left = dpp_lower(t1);   // t at column y0-1 (lane-1's second column)
    const double right = dpp_upper(t0);  // t at column y0+2 (lane+1's first column)
    o0 = w.dm0 + ((left + t1) + q0);
    o1 = w.dm1 + ((t0 + right) + q1);
    w.sa0 = w.sm0;
    w.sa1 = w.sm1;
    w.sm0 = sn0;
    w.sm1 = sn1;
    w.dm0 = dn0;
    w.dm1 = dn1;
}

// The per-wave buffers of one pass: input rows rA-K .. rB+K-1 of the state and of the rate
// field, output rows rA .. rB-1.
template <int K>
struct FBufs {
    __amdgpu_buffer_rsrc_t in, fld, out;
    __device__ __forceinline__ FBufs(const PassArgs& A, int rA, int rB) {
        in = rows_rsrc(A.in[0] + (long long)(rA - K) * A.pitch, rB - rA + 2 * K, A.pitch);
        fld = rows_rsrc(A.field[0] + (long long)(rA - K) * A.pitch, rB - rA + 2 * K, A.pitch);
        out = rows_rsrc(A.out[0] + (long long)rA * A.pitch, rB - rA, A.pitch);
    }
};

// Steady state, iterations [b0, b1) (b0 = I0 mod the ring, b1 - b0 a multiple of it): every
// level emits one row per iteration, level K's row rA + (i - I0) is stored. FAST: every row
// the levels read in these iterations is an interior row of an interior strip.
template <int K, bool RED, int NT, bool FAST>
__device__ __forceinline__ void fk_steady(const Lane& c, const FBufs<K>& B, int rA, int rB,
                                          unsigned voff, unsigned soff, unsigned rowb, int b0,
                                          int b1, dv2 (&rawv)[kFieldPrefetch],
                                          dv2 (&rawf)[field_ring(K)], FWin (&win)[K],
                                          double (&pend0)[K], double (&pend1)[K],
                                          double (&acc)[K][1]) {
    constexpr int I0 = 3 * K - 1, U = kFieldPrefetch, LF = field_ring(K);
    for (int base = b0; base < b1; base += LF) {
#pragma unroll
        for (int t = 0; t < LF; ++t) {
            const int i = base + t;
#pragma unroll
            for (int j = K; j >= 1; --j) {  // descending: pend[j-2] is read before it is refilled
                constexpr int kBack = 2 * (K - 1);
                const int fslot = (I0 + t - 2 * (j - 1)) % LF;  // base = I0 (mod LF)
                double v0, v1;
                if (j == 1) {
                    const int vslot = (I0 + t) % U;
                    v0 = vcopy(rawv[vslot].x);
                    v1 = vcopy(rawv[vslot].y);
                    rawv[vslot] = load_row(B.in, voff + (unsigned)(i + U) * rowb);
                } else {
                    v0 = pend0[j - 2];
                    v1 = pend1[j - 2];
                }
                const long long gx = c.gx0 + rA - K + i - 2 * (j - 1);
                double w0, w1;
                fk_emit<FAST>(c, gx, win[j - 1], v0, v1, rawf[fslot].x, rawf[fslot].y, w0, w1);
                // level K was the last reader of its rate row: the slot takes the row a ring ahead
                if (j == K) rawf[fslot] = load_row(B.fld, voff + (unsigned)(i - kBack + LF) * rowb);
                const int r = rA - K - 2 * j + 1 + i;  // output row
                if (RED) accum(acc[j - 1][0], r >= rA && r < rB, c, w0, w1);
                if (j == K) {
                    store_row<NT>(B.out, soff + (unsigned)(r - rA) * rowb, w0, w1);
                } else {
                    pend0[j - 1] = w0;
                    pend1[j - 1] = w1;
                }
            }
            __builtin_amdgcn_sched_barrier(0);  // keep the row order: bounds the live registers
        }
    }
}

// One segment: R = rB - rA rows (run time). Iterations 0 .. 3K-2 fill the levels
// (compile-time); from iteration I0 = 3K-1 on every level emits, and the loop runs R
// iterations rounded up to the ring (the extra ones read zeros past the input rows and
// their stores fall past the output rows). A wave of an interior strip whose segment
// touches the grid's first or last rows runs the general body only for the iterations that
// read those rows.
template <int K, bool RED, int NT, bool FAST>
__device__ __forceinline__ void fieldk_segment(const PassArgs& A, const Lane& c, long long wid,
                                               int lane, int rA, int rB, unsigned voff,
                                               unsigned soff) {
    constexpr int I0 = 3 * K - 1, U = kFieldPrefetch, LF = field_ring(K);
    static_assert(I0 <= LF, "the prologue reloads no rate slot twice");
    const int R = rB - rA;
    double acc[K][1];
#pragma unroll
    for (int j = 0; j < K; ++j) acc[j][0] = 0.0;
    const unsigned rowb = (unsigned)(A.pitch * 8);
    const FBufs<K> B(A, rA, rB);
    dv2 rawv[U], rawf[LF];
#pragma unroll
    for (int k = 0; k < LF; ++k) {
        if (k < U) rawv[k] = load_row(B.in, voff + k * rowb);
        rawf[k] = load_row(B.fld, voff + k * rowb);
    }
    FWin win[K];
    double pend0[K], pend1[K];

    // prologue: level j takes part from iteration 3(j-1); nothing is stored yet
#pragma unroll
    for (int i = 0; i < I0; ++i) {
#pragma unroll
        for (int j = K; j >= 1; --j) {
            const int m = i - 3 * (j - 1);
            if (m < 0) continue;  // compile-time
            const int fslot = (i - 2 * (j - 1)) % LF;
            double v0, v1;
            if (j == 1) {
                v0 = rawv[i % U].x;
                v1 = rawv[i % U].y;
                rawv[i % U] = load_row(B.in, voff + (i + U) * rowb);
            } else {
                v0 = pend0[j - 2];
                v1 = pend1[j - 2];
            }
            const long long gx = c.gx0 + rA - K + (j - 1) + m;
            if (m < 2) {
                fk_fill<FAST>(c, gx, m, win[j - 1], v0, v1, rawf[fslot].x, rawf[fslot].y);
                continue;
            }
            double w0, w1;
            fk_emit<FAST>(c, gx, win[j - 1], v0, v1, rawf[fslot].x, rawf[fslot].y, w0, w1);
            const int r = rA - K - 2 * j + 1 + i;  // output row
            if (RED) accum(acc[j - 1][0], r >= rA && r < rB, c, w0, w1);
            pend0[j - 1] = w0;  // j < K here: level K's m <= 1 in the prologue
            pend1[j - 1] = w1;
        }
        // input row i - 2(K-1) has had its last reader (level K, or no level at all: level
        // j's first input row is row j-1)
        if (i - 2 * (K - 1) >= 0)
            rawf[(i - 2 * (K - 1)) % LF] = load_row(B.fld, voff + (i - 2 * (K - 1) + LF) * rowb);
        __builtin_amdgcn_sched_barrier(0);
    }

    const int end = I0 + (R + LF - 1) / LF * LF;
    if (FAST) {
        fk_steady<K, RED, NT, true>(c, B, rA, rB, voff, soff, rowb, I0, end, rawv, rawf, win, pend0,
                                    pend1, acc);
    } else {
        int f0 = end, f1 = end;  // iterations [f0, f1) read interior rows only
        if (c.fast_cols) {
            // iteration i: the levels read global rows g - 2(K-1) .. g, g = gx0 + rA - K + i
            const long long g0 = c.gx0 + rA - K;
            const long long lo = 1 + 2 * (K - 1) - g0;  // first i with every row >= 1
            const long long hi = c.H - 1 - g0;          // first i with a row > H-2
            const long long a0 = lo <= I0 ? I0 : I0 + (lo - I0 + LF - 1) / LF * LF;
            const long long a1 = hi <= I0 ? I0 : I0 + (hi - I0) / LF * LF;
            f0 = (int)min((long long)end, a0);
            f1 = (int)max((long long)f0, min((long long)end, a1));
        }
        fk_steady<K, RED, NT, false>(c, B, rA, rB, voff, soff, rowb, I0, f0, rawv, rawf, win, pend0,
                                     pend1, acc);
        fk_steady<K, RED, NT, true>(c, B, rA, rB, voff, soff, rowb, f0, f1, rawv, rawf, win, pend0,
                                    pend1, acc);
        fk_steady<K, RED, NT, false>(c, B, rA, rB, voff, soff, rowb, f1, end, rawv, rawf, win, pend0,
                                     pend1, acc);
    }
    if (RED) write_sums<K, 1>(A, wid, lane, acc);
}

// BLOCK schedule (mm_passk.hpp passk_block): TH output rows, the border rows of a halo-split
// pass. Every one of the TH + 3K - 1 iterations is unrolled at compile time: level fill
// states, row offsets and block ownership are constants, and so is the rate row of every
// level -- the TH + 2K rate rows are loaded once and stay in registers (4 VGPRs per row and
// lane), no ring, no reload. Level j's m-th input is row (j-1) + m of the block's input rows
// rA-K .. rA+TH+K-1. A block cut short by the range's end (rB < rA + TH) reads zeros past
// its descriptors; the rows past rB are neither stored nor summed.
template <int K, int TH, bool RED, bool FAST>
__device__ __forceinline__ void fieldk_block(const PassArgs& A, const Lane& c, long long wid,
                                             int lane, int rA, int rB, unsigned voff,
                                             unsigned soff) {
    constexpr int NI = TH + 2 * K;       // input rows
    constexpr int NIT = TH + 3 * K - 1;  // iterations
    constexpr int U = 4;                 // state rows prefetched
    double acc[K][1];
#pragma unroll
    for (int j = 0; j < K; ++j) acc[j][0] = 0.0;
    const unsigned rowb = (unsigned)(A.pitch * 8);
    const FBufs<K> B(A, rA, rB);
    dv2 rawv[U], rawf[NI];
#pragma unroll
    for (int k = 0; k < NI; ++k) {
        if (k < U) rawv[k] = load_row(B.in, voff + k * rowb);
        rawf[k] = load_row(B.fld, voff + k * rowb);
    }
    FWin win[K];
    double pend0[K], pend1[K];  // level j's row of the previous iteration: pend[j-1]

#pragma unroll
    for (int i = 0; i < NIT; ++i) {
#pragma unroll
        for (int j = K; j >= 1; --j) {  // descending: pend[j-2] is read before it is refilled
            const int m = i - 3 * (j - 1);
            if (m < 0 || m >= NI - 2 * (j - 1)) continue;  // compile-time
            double v0, v1;
            if (j == 1) {
                v0 = rawv[i % U].x;
                v1 = rawv[i % U].y;
                if (i + U < NI) rawv[i % U] = load_row(B.in, voff + (i + U) * rowb);
            } else {
                v0 = pend0[j - 2];
                v1 = pend1[j - 2];
            }
            const int row = (j - 1) + m;  // of the block's input rows: the level's rate row
            const long long gx = c.gx0 + rA - K + row;
            if (m < 2) {
                fk_fill<FAST>(c, gx, m, win[j - 1], v0, v1, rawf[row].x, rawf[row].y);
                continue;
            }
            double w0, w1;
            fk_emit<FAST>(c, gx, win[j - 1], v0, v1, rawf[row].x, rawf[row].y, w0, w1);
            const int orow = m + j - K - 2;  // output row - rA (compile-time)
            if (RED && orow >= 0 && orow < TH) accum(acc[j - 1][0], rA + orow < rB, c, w0, w1);
            if (j == K) {
                store_row<0>(B.out, soff + orow * rowb, w0, w1);
            } else {
                pend0[j - 1] = w0;
                pend1[j - 1] = w1;
            }
        }
        __builtin_amdgcn_sched_barrier(0);  // keep the row order: bounds the live registers
    }
    if (RED) write_sums<K, 1>(A, wid, lane, acc);
}

// K steps of a one-attribute rate-field diffusion per launch. MODE: kSeg = segment schedule
// (A.th / A.th_edge rows per wave, mm_passk.hpp seg_map), else the block schedule with MODE
// rows per wave (the border rows of a halo-split pass). The wave map is mm_passk_kernel's:
// waves below A.waves_a work in rows [ra0, ra1), the others in [rb0, rb1). RED: per-level
// sums of the owned cells into partials[(partial_base + wave) * K + level]. NT & 1:
// non-temporal stores (segment schedule). Two waves per SIMD at least: 256 registers per lane.
template <int K, int MODE, bool RED, int NT>
__global__ __launch_bounds__(kBlock, 2) void mm_fieldk_kernel(const PassArgs A) {
    static_assert(K >= 2 && K <= kFieldMaxSteps, "mm_geom.hpp: kFieldMaxSteps");
    constexpr int L = (K + 1) / 2;          // halo lanes per side
    constexpr int OC = kStripCols - 4 * L;  // output columns per strip
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long wid = (long long)blockIdx.x * kWavesPerBlock + wave;
    if (wid >= A.waves_total) return;

    int rlo, rhi;
    long long w = wid;
    if (w < A.waves_a) {
        rlo = A.ra0;
        rhi = A.ra1;
    } else {
        w -= A.waves_a;
        rlo = A.rb0;
        rhi = A.rb1;
    }
    int strip, rA, rB;
    if (MODE == kSeg) {
        seg_map(w, rlo, rhi, A.nstrips, A.th, A.th_edge, strip, rA, rB);
    } else {
        strip = (int)(w % A.nstrips);
        rA = rlo + (int)(w / A.nstrips) * MODE;
        rB = min(rA + MODE, rhi);
    }

    const long long W = A.W;
    const long long c0 = (long long)strip * OC - 2 * L;  // first loaded column (even)
    const long long y0 = c0 + 2 * lane;
    const bool in_row = y0 >= 0 && y0 < A.pitch;  // y0 even, pitch a multiple of 128
    const unsigned voff = in_row ? (unsigned)(y0 * 8) : kOOB;
    const bool store_lane = lane >= L && lane < 64 - L && y0 < W;
    // columns past W inside the pitch are padding: writing them is harmless
    const unsigned soff = store_lane ? (unsigned)(y0 * 8) : kOOB;
    Lane c;
    c.H = A.H;
    c.gx0 = A.x_init;
    c.sy0 = span3(W, y0);
    c.sy1 = span3(W, y0 + 1);
    c.fast_cols = c0 >= 1 && c0 + kStripCols <= W - 1;  // loaded cols in [1, W-2]
    c.own0 = store_lane;
    c.own1 = store_lane && y0 + 1 < W;
    c.from_lower = c.from_upper = 0;

    // a wave whose input rows and loaded columns are all interior (cnt == 8 everywhere)
    // runs the branch-free body; edge waves run the general one
    const bool fast = c.fast_cols && c.gx0 + rA - K >= 1 && c.gx0 + rB + K - 1 <= A.H - 2;
    if constexpr (MODE == kSeg) {
        if (fast)
            fieldk_segment<K, RED, NT, true>(A, c, wid, lane, rA, rB, voff, soff);
        else
            fieldk_segment<K, RED, NT, false>(A, c, wid, lane, rA, rB, voff, soff);
    } else {
        if (fast)
            fieldk_block<K, MODE, RED, true>(A, c, wid, lane, rA, rB, voff, soff);
        else
            fieldk_block<K, MODE, RED, false>(A, c, wid, lane, rA, rB, voff, soff);
    }
}

// The instances of one K: the segment schedule with or without non-temporal stores, the
// border blocks of kBorderRows rows (q.nt does not apply), each with the step sums or
// without. nullptr for another kernel's key.
template <int K>
const KernelInst* fieldk_inst(const InstKey& q) {
    if (q.family != kInstFieldK || q.k != K || q.na != 1 || q.cols != 2) return nullptr;
    if (!q.seg)
        return q.red ? inst_of<mm_fieldk_kernel<K, kBorderRows, true, 0>, kBlock>()
                     : inst_of<mm_fieldk_kernel<K, kBorderRows, false, 0>, kBlock>();
    if (q.nt)
        return q.red ? inst_of<mm_fieldk_kernel<K, kSeg, true, 1>, kBlock>()
                     : inst_of<mm_fieldk_kernel<K, kSeg, false, 1>, kBlock>();
    return q.red ? inst_of<mm_fieldk_kernel<K, kSeg, true, 0>, kBlock>()
                 : inst_of<mm_fieldk_kernel<K, kSeg, false, 0>, kBlock>();
}

}  // namespace

}  // namespace mm
