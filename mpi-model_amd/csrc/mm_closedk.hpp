// mm_closedk.hpp -- K fused steps of the closed rate-field diffusion (MM_FLOW_DIFFUSE_CLOSED)
// per HBM pass, gfx950: temporal blocking of mm_closed_kernel's step for a program that is one
// closed diffusion of one attribute on a slab without a halo. A pass reads every cell's value
// and rate once, advances the value K steps in registers and writes it once: 24/K B per
// cell-update instead of 24 B. No extra HBM stream: openness and counts are rebuilt from the
// rate rows the pass reads anyway.
//
// The schedule is mm_fieldk_kernel's SEGMENT schedule (mm_fieldk.hpp, mm_passk.hpp): a wave per
// strip of 128 loaded columns (lane l: columns c0+2l, c0+2l+1 as one 16-B buffer load per
// row), the K levels skewed (at iteration i level j consumes input row i - 2(j-1) of the
// segment), a per-level window of s, s, d, the pend hand-off between levels, one rows_rsrc
// descriptor per wave and buffer, the register ring for the rate rows, a sched_barrier per row
// and per-level partials through write_sums. On a slab with a halo the interior rows run that
// schedule beside the exchange and the K border rows of each side the BLOCK schedule after it
// (closedk_block below, the counterpart of mm_fieldk.hpp's fieldk_block), which reads K ghost
// rows of the state and K + 1 of the rate field (MM_CLOSED_HALO, include/mpimodel.h).
//
// The dependency cone. K steps of a cell read v within Chebyshev distance K and f within
// K + 1: the share a cell at distance K gives at step 1 needs that cell's count of open
// neighbours. So a segment of output rows [rA, rB) reads v of rows rA-K .. rB+K-1 and f of rows
// rA-K-1 .. rB+K, and a strip that loads columns [c0, c0+128) knows the count only of columns
// c0+1 .. c0+126: what it computes for column c0 is garbage from level 1 on, and the garbage
// moves one column inward per level, so level K is valid from column c0+K+1.
// Columns: the discarded halo is widened to L = floor((K+2)/2) lanes (2L >= K+1 columns) a
// side -- closedk_out_cols(K), mm_geom.hpp -- one lane more than mm_fieldk_kernel at K = 2
// and 4, the same at K = 3. The alternative, edge lanes that load the column beside the strip
// as mm_closed_kernel's lanes 0 and 63 do, would add a second load per row and lane, a third
// column to every level's share and window in all 64 lanes (the wave executes what its edge
// lanes execute) and the tied-old DPP shifts; the wider halo costs 4 of 128 (L2-resident)
// columns and keeps every lane on the same instructions.
//
// Openness does not depend on the step. When a rate row enters (one iteration before level 1
// consumes it, so f runs one row ahead of v) it becomes two open bits per lane, closed by
// select where the row is outside the grid or the column outside [0, W); the bits of the +-1
// columns come through DPP shifts and add up to column triples, a byte per column
// (mm_closed.hip); the triples of three rows add up to the 3 x 3 box (one 32-bit add: no byte
// exceeds 9). The ring keeps, beside the four registers of a row's f, one register with the
// row's box bytes and own bits: level j reads cnt = box - own at its skewed iteration instead
// of rebuilding it. The ring is closed_ring(K) rows (mm_geom.hpp).
// Two wave-uniform choices are made once per row, when its box is known, and kept as a scalar
// beside the ring slot: every column whose count the wave knows has a box byte of 9 (the row
// takes the division-free body at every level: s = out * 0.125, no select), or nothing in the
// row emits (every share is 0, no multiplication); every other row runs share_one (the IEEE
// division; walls and cnt == 0 by select). Which body runs is decided from the data alone.
//
// Arithmetic: each level is mm_closed.hip's step, operation for operation (header comment
// there; -ffp-contract=off), so K fused steps are bit-identical to K single steps. A wall
// keeps v bit for bit at every level, by select; it may hold NaN, an infinity or -0, and so
// may the pitch padding and the ghost rows of v and f.
//
// This header holds the kernel template; mm_closedk_k<K>.hip instantiate it (one translation
// unit per K) and mm_kernels_k.hip dispatches.
#pragma once

#include "mm_passk.hpp"

namespace mm {

namespace {

// the wave shifts on a 32-bit word; lanes without a source lane read 0 (a closed column)
__device__ __forceinline__ int ck_lower(int src) {
    return __builtin_amdgcn_mov_dpp(src, 0x138, 0xf, 0xf, true);  // wave_shr:1
}
__device__ __forceinline__ int ck_upper(int src) {
    return __builtin_amdgcn_mov_dpp(src, 0x130, 0xf, 0xf, true);  // wave_shl:1
}

// the row-uniform body choice
constexpr int kRowGen = 0, kRowAll8 = 1, kRowNone = 2;
// a ring row's word: box bytes of the lane's two columns, then their own bits
constexpr int kOwn0 = 1 << 16, kOwn1 = 1 << 17;

// What a lane knows of its place.
struct CKLane {
    long long H, gx0;  // grid rows, global row of local row 0
    bool in0, in1;     // own columns inside the grid
    bool own0, own1;   // own columns are output cells of this wave
    int known;         // byte mask of the columns whose count the wave knows (all but the
                       // first column of lane 0 and the last of lane 63)
};

// One level's three-row window: the shares of the row above (sa) and of the current row
// (sm), the current row's d = v - out (dm; v itself for a wall).
struct CKWin {
    double sa0, sa1, sm0, sm1, dm0, dm1;
};

// A rate row turned into openness: the lane's two open bits and the column triples (open
// cells among columns y-1..y+1, a byte per column). rin: the row is inside the grid.
__device__ __forceinline__ void ck_open(const CKLane& c, long long gx, dv2 f, int& ob, int& tri) {
    const bool rin = gx >= 0 && gx < c.H;
    const int b0 = (rin && c.in0 && f.x != 0.0) ? 1 : 0;
    const int b1 = (rin && c.in1 && f.y != 0.0) ? 1 : 0;
    ob = b0 | b1 << 1;
    const int left = (ck_lower(ob) >> 1) & 1;  // column y0-1: the lower lane's second column
    const int right = ck_upper(ob) & 1;        // column y0+2: the upper lane's first column
    tri = (left + b0 + b1) | (b0 + b1 + right) << 8;
}

// The ring word of a row and its body choice from the triples of the rows above and below,
// its own triples and its own bits.
__device__ __forceinline__ void ck_box(const CKLane& c, int tri_up, int tri, int tri_dn, int ob,
                                       int& word, int& mode) {
    const int box = tri_up + tri + tri_dn;
    const int b0 = ob & 1, b1 = (ob >> 1) & 1;
    const bool all8 = (box & c.known) == (0x0909 & c.known);
    const bool emits = ((box & c.known & 0xff) > 1 && b0) || (((box & c.known) >> 8) > 1 && b1);
    word = box | ob << 16;
    const bool a = __builtin_amdgcn_ballot_w64(all8) == ~0ull;
    const bool n = __builtin_amdgcn_ballot_w64(emits) == 0ull;
    mode = __builtin_amdgcn_readfirstlane(a ? kRowAll8 : (n ? kRowNone : kRowGen));
}

// Shares and d of this lane's two columns of a row (mm_closed.hip cshare_row).
__device__ __forceinline__ void ck_share(int mode, int word, double v0, double v1, double f0,
                                         double f1, double& s0, double& s1, double& d0,
                                         double& d1) {
    const bool b0 = (word & kOwn0) != 0, b1 = (word & kOwn1) != 0;
    if (mode == kRowAll8) {  // row-uniform: no division, no select
        const double out0 = f0 * v0, out1 = f1 * v1;
        s0 = out0 * 0.125;
        s1 = out1 * 0.125;
        d0 = v0 - out0;
        d1 = v1 - out1;
    } else if (mode == kRowNone) {  // walls and lone cells only
        s0 = s1 = 0.0;
        d0 = b0 ? v0 - 0.0 : v0;
        d1 = b1 ? v1 - 0.0 : v1;
    } else {
        double out0, out1;
        share_one(v0, f0, b0, (word & 0xff) - (b0 ? 1 : 0), out0, s0);
        share_one(v1, f1, b1, ((word >> 8) & 0xff) - (b1 ? 1 : 0), out1, s1);
        d0 = b0 ? v0 - out0 : v0;
        d1 = b1 ? v1 - out1 : v1;
    }
}

// Level input row m = 0 or 1: fill the window.
__device__ __forceinline__ void ck_fill(int m, CKWin& w, int mode, int word, double v0, double v1,
                                        double f0, double f1) {
    double s0, s1, d0, d1;
    ck_share(mode, word, v0, v1, f0, f1, s0, s1, d0, d1);
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

// Level input row m >= 2: emit the window's current row (mm_closed.hip cemit_row; wordm: its
// ring word, a wall keeps d = v) and slide the window.
__device__ __forceinline__ void ck_emit(CKWin& w, int mode, int word, int wordm, double v0,
                                        double v1, double f0, double f1, double& o0, double& o1) {
    double sn0, sn1, dn0, dn1;
    ck_share(mode, word, v0, v1, f0, f1, sn0, sn1, dn0, dn1);
    const double q0 = w.sa0 + sn0, q1 = w.sa1 + sn1;
    const double t0 = q0 + w.sm0, t1 = q1 + w.sm1;
    const double left = dpp_lower(t1);   // t at column y0-1 (lane-1's second column)
    const double right = dpp_upper(t0);  // t at column y0+2 (lane+1's first column)
    o0 = (wordm & kOwn0) ? w.dm0 + ((left + t1) + q0) : w.dm0;
    o1 = (wordm & kOwn1) ? w.dm1 + ((t0 + right) + q1) : w.dm1;
    w.sa0 = w.sm0;
    w.sa1 = w.sm1;
    w.sm0 = sn0;
    w.sm1 = sn1;
    w.dm0 = dn0;
    w.dm1 = dn1;
}

__device__ __forceinline__ void ck_accum(double& acc, bool own, const CKLane& c, double w0,
                                         double w1) {
    acc = acc + ((own && c.own0) ? w0 : 0.0);
    acc = acc + ((own && c.own1) ? w1 : 0.0);
    asm volatile("" : "+v"(acc));
}

// The per-wave buffers of one pass: input rows rA-K .. rB+K-1 of the state, rows rA-K-1 ..
// rB+K of the rate field (row k of the state is row k+1 of the field's range), output rows
// rA .. rB-1.
template <int K>
struct CKBufs {
    __amdgpu_buffer_rsrc_t in, fld, out;
    __device__ __forceinline__ CKBufs(const PassArgs& A, int rA, int rB) {
        in = rows_rsrc(A.in[0] + (long long)(rA - K) * A.pitch, rB - rA + 2 * K, A.pitch);
        fld = rows_rsrc(A.field[0] + (long long)(rA - K - 1) * A.pitch, rB - rA + 2 * K + 2,
                        A.pitch);
        out = rows_rsrc(A.out[0] + (long long)rA * A.pitch, rB - rA, A.pitch);
    }
};

// The rate ring and the openness that rolls ahead of level 1. Slot of input row n (row n+1
// of the field's range): (n + 1) % LF.
template <int K>
struct CKRing {
    static constexpr int LF = closed_ring(K);
    dv2 f[LF];
    int word[LF], mode[LF];
    int tri_a, tri_b, ob_b;  // triples of input rows i-1 and i, own bits of row i
};

// Iteration i, before the levels: input row i+1's rates become openness, which completes the
// box of input row i. slot1 / slot2: the ring slots of input rows i and i+1.
template <int K>
__device__ __forceinline__ void ck_enter(const CKLane& c, long long gx, CKRing<K>& R, int slot1,
                                         int slot2) {
    int ob_n, tri_n;
    ck_open(c, gx + 1, R.f[slot2], ob_n, tri_n);
    ck_box(c, R.tri_a, R.tri_b, tri_n, R.ob_b, R.word[slot1], R.mode[slot1]);
    R.tri_a = R.tri_b;
    R.tri_b = tri_n;
    R.ob_b = ob_n;
}

// One segment: R = rB - rA rows (run time). Iterations 0 .. 3K-2 fill the levels
// (compile-time); from iteration I0 = 3K-1 on every level emits, level K's row rA + (i - I0)
// is stored, and the loop runs R iterations rounded up to the ring, unrolled once around it
// (the extra ones read zeros past the input rows and their stores fall past the output rows).
template <int K, bool RED, int NT>
__device__ __forceinline__ void closedk_segment(const PassArgs& A, const CKLane& c, long long wid,
                                                int lane, int rA, int rB, unsigned voff,
                                                unsigned soff) {
    constexpr int I0 = 3 * K - 1, U = kFieldPrefetch, LF = closed_ring(K);
    constexpr int kBack = 2 * (K - 1);
    static_assert(I0 <= LF, "the prologue reloads no rate slot twice");
    static_assert(U + kBack + 2 <= LF + 1, "a slot is reloaded U rows or more ahead of its entry");
    const int R = rB - rA;
    double acc[K][1];
#pragma unroll
    for (int j = 0; j < K; ++j) acc[j][0] = 0.0;
    const unsigned rowb = (unsigned)(A.pitch * 8);
    const CKBufs<K> B(A, rA, rB);
    const long long g0 = c.gx0 + rA - K;  // global row of input row 0
    dv2 rawv[U];
    CKRing<K> G;
#pragma unroll
    for (int k = 0; k < LF; ++k) {
        if (k < U) rawv[k] = load_row(B.in, voff + k * rowb);
        G.f[k] = load_row(B.fld, voff + k * rowb);
    }
    {
        int ob_a;
        ck_open(c, g0 - 1, G.f[0], ob_a, G.tri_a);
        (void)ob_a;
        ck_open(c, g0, G.f[1], G.ob_b, G.tri_b);
    }
    CKWin win[K];
    double pend0[K], pend1[K];

    // prologue: level j takes part from iteration 3(j-1); nothing is stored yet
#pragma unroll
    for (int i = 0; i < I0; ++i) {
        ck_enter<K>(c, g0 + i, G, (i + 1) % LF, (i + 2) % LF);
#pragma unroll
        for (int j = K; j >= 1; --j) {
            const int m = i - 3 * (j - 1);
            if (m < 0) continue;  // compile-time
            const int n = i - 2 * (j - 1);  // the level's input row
            const int fslot = (n + 1) % LF;
            double v0, v1;
            if (j == 1) {
                v0 = rawv[i % U].x;
                v1 = rawv[i % U].y;
                rawv[i % U] = load_row(B.in, voff + (i + U) * rowb);
            } else {
                v0 = pend0[j - 2];
                v1 = pend1[j - 2];
            }
            if (m < 2) {
                ck_fill(m, win[j - 1], G.mode[fslot], G.word[fslot], v0, v1, G.f[fslot].x,
                        G.f[fslot].y);
                continue;
            }
            double w0, w1;
            ck_emit(win[j - 1], G.mode[fslot], G.word[fslot], G.word[n % LF], v0, v1, G.f[fslot].x,
                    G.f[fslot].y, w0, w1);
            const int r = rA - K - 2 * j + 1 + i;  // output row
            if (RED) ck_accum(acc[j - 1][0], r >= rA && r < rB, c, w0, w1);
            pend0[j - 1] = w0;  // j < K here: level K's m <= 1 in the prologue
            pend1[j - 1] = w1;
        }
        // input row i - 2(K-1) has had its last reader (level K, or no level at all; row -1:
        // the box of row 0): its slot takes the row a ring ahead
        if (i - kBack + 1 >= 0)
            G.f[(i - kBack + 1) % LF] = load_row(B.fld, voff + (i - kBack + 1 + LF) * rowb);
        __builtin_amdgcn_sched_barrier(0);
    }

    const int end = I0 + (R + LF - 1) / LF * LF;
    for (int base = I0; base < end; base += LF) {
#pragma unroll
        for (int t = 0; t < LF; ++t) {
            const int i = base + t;
            ck_enter<K>(c, g0 + i, G, (I0 + t + 1) % LF, (I0 + t + 2) % LF);  // base = I0 (mod LF)
#pragma unroll
            for (int j = K; j >= 1; --j) {  // descending: pend[j-2] is read before it is refilled
                const int nn = I0 + t - 2 * (j - 1);  // the level's input row (mod LF)
                const int fslot = (nn + 1) % LF;
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
                double w0, w1;
                ck_emit(win[j - 1], G.mode[fslot], G.word[fslot], G.word[nn % LF], v0, v1,
                        G.f[fslot].x, G.f[fslot].y, w0, w1);
                // level K was the last reader of its rate row: the slot takes the row a ring ahead
                if (j == K) G.f[fslot] = load_row(B.fld, voff + (unsigned)(i - kBack + 1 + LF) * rowb);
                const int r = rA - K - 2 * j + 1 + i;  // output row
                if (RED) ck_accum(acc[j - 1][0], r >= rA && r < rB, c, w0, w1);
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
    if (RED) write_sums<K, 1>(A, wid, lane, acc);
}

// BLOCK schedule (mm_fieldk.hpp fieldk_block): TH output rows [rA, rB), the border rows of a
// halo-split pass. Every one of the TH + 3K - 1 iterations is unrolled at compile time, so level
// fill states, row offsets and block ownership are constants. There is no ring: the TH + 2K + 2
// rate rows rA-K-1 .. rA+TH+K are loaded once and stay in registers (4 VGPRs per row and lane),
// and the openness is built once, up front -- ck_open per rate row, ck_box per input row: TH + 2K
// ring words and as many scalar body choices. Level j's m-th input is row (j-1) + m of the
// block's input rows rA-K .. rA+TH+K-1, with that row's f, word and mode; the level itself is
// ck_fill / ck_emit, so a block computes what a segment does, bit for bit. A block cut short by
// the range's end (rB < rA + TH) reads zeros -- closed rows -- past its descriptors; the rows
// past rB are neither stored nor summed.
template <int K, int TH, bool RED>
__device__ __forceinline__ void closedk_block(const PassArgs& A, const CKLane& c, long long wid,
                                              int lane, int rA, int rB, unsigned voff,
                                              unsigned soff) {
    constexpr int NI = TH + 2 * K;       // input rows of the state
    constexpr int NF = NI + 2;           // rate rows: row k is input row k - 1
    constexpr int NIT = TH + 3 * K - 1;  // iterations
    constexpr int U = 4;                 // state rows prefetched
    double acc[K][1];
#pragma unroll
    for (int j = 0; j < K; ++j) acc[j][0] = 0.0;
    const unsigned rowb = (unsigned)(A.pitch * 8);
    const CKBufs<K> B(A, rA, rB);
    const long long g0 = c.gx0 + rA - K;  // global row of input row 0
    dv2 rawv[U], rawf[NF];
#pragma unroll
    for (int k = 0; k < NF; ++k) {
        if (k < U) rawv[k] = load_row(B.in, voff + k * rowb);
        rawf[k] = load_row(B.fld, voff + k * rowb);
    }
    int word[NI], mode[NI];
    {
        int ob[NF], tri[NF];
#pragma unroll
        for (int k = 0; k < NF; ++k) ck_open(c, g0 - 1 + k, rawf[k], ob[k], tri[k]);
#pragma unroll
        for (int n = 0; n < NI; ++n)
            ck_box(c, tri[n], tri[n + 1], tri[n + 2], ob[n + 1], word[n], mode[n]);
    }
    CKWin win[K];
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
            const int row = (j - 1) + m;  // of the block's input rows; its rates: rawf[row + 1]
            if (m < 2) {
                ck_fill(m, win[j - 1], mode[row], word[row], v0, v1, rawf[row + 1].x,
                        rawf[row + 1].y);
                continue;
            }
            double w0, w1;
            ck_emit(win[j - 1], mode[row], word[row], word[row - 1], v0, v1, rawf[row + 1].x,
                    rawf[row + 1].y, w0, w1);
            const int orow = m + j - K - 2;  // output row - rA (compile-time)
            if (RED && orow >= 0 && orow < TH) ck_accum(acc[j - 1][0], rA + orow < rB, c, w0, w1);
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

// K steps of a one-attribute closed rate-field diffusion per launch. MODE: kSeg = segment
// schedule (A.th / A.th_edge rows per wave, mm_passk.hpp seg_map), else the block schedule with
// MODE rows per wave (the border rows of a halo-split pass). The wave map is mm_passk_kernel's:
// waves below A.waves_a work in rows [ra0, ra1), the others in [rb0, rb1). RED: per-level sums
// of the owned cells, walls included, into partials[(partial_base + wave) * K + level]. NT & 1:
// non-temporal stores (segment schedule). Two waves per SIMD at least: 256 registers per lane.
template <int K, int MODE, bool RED, int NT>
__global__ __launch_bounds__(kBlock, 2) void mm_closedk_kernel(const PassArgs A) {
    static_assert(K >= 2 && K <= kClosedMaxSteps, "mm_geom.hpp: kClosedMaxSteps");
    constexpr int L = (K + 2) / 2;            // halo lanes per side: 2L >= K + 1 columns
    constexpr int OC = closedk_out_cols(K);   // output columns per strip
    static_assert(OC == kStripCols - 4 * L && 2 * L >= K + 1, "mm_geom.hpp: closedk_out_cols");
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
    CKLane c;
    c.H = A.H;
    c.gx0 = A.x_init;
    c.in0 = y0 >= 0 && y0 < W;
    c.in1 = y0 >= 0 && y0 + 1 < W;
    c.own0 = store_lane;
    c.own1 = store_lane && y0 + 1 < W;
    c.known = lane == 0 ? 0xff00 : (lane == 63 ? 0x00ff : 0xffff);
    if constexpr (MODE == kSeg)
        closedk_segment<K, RED, NT>(A, c, wid, lane, rA, rB, voff, soff);
    else
        closedk_block<K, MODE, RED>(A, c, wid, lane, rA, rB, voff, soff);
}

// The instances of one K: the segment schedule with or without non-temporal stores, the
// border blocks of kBorderRows rows (q.nt does not apply), each with the step sums or
// without. nullptr for another kernel's key.
template <int K>
const KernelInst* closedk_inst(const InstKey& q) {
    if (q.family != kInstClosedK || q.k != K || q.na != 1 || q.cols != 2) return nullptr;
    if (!q.seg)
        return q.red ? inst_of<mm_closedk_kernel<K, kBorderRows, true, 0>, kBlock>()
                     : inst_of<mm_closedk_kernel<K, kBorderRows, false, 0>, kBlock>();
    if (q.nt)
        return q.red ? inst_of<mm_closedk_kernel<K, kSeg, true, 1>, kBlock>()
                     : inst_of<mm_closedk_kernel<K, kSeg, false, 1>, kBlock>();
    return q.red ? inst_of<mm_closedk_kernel<K, kSeg, true, 0>, kBlock>()
                 : inst_of<mm_closedk_kernel<K, kSeg, false, 0>, kBlock>();
}

}  // namespace

}  // namespace mm
