// mm_field.hip -- gfx950 kernel of the rate-field diffusion (MM_FLOW_DIFFUSE_FIELD): the
// reference's per-emitter Exponencial update (src/Model.hpp:199,206-211,234) with a rate
// that is a per-cell map f, one step per pass.
//
// Arithmetic contract (include/mpimodel.h; bit for bit or_field_step_general of
// oracle/mm_oracle.c with outf = f * v). For the in-grid cell c = (x, y) with cnt(c)
// in-grid Moore neighbours:
//   out(c) = f(c) * v(c)              if cnt(c) > 0, else 0
//   s(c)   = out(c) * 0.125           if cnt(c) == 8
//            out(c) / (double)cnt(c)  otherwise          (0 for any cell outside the grid)
//   q(x,y) = s(x-1,y) + s(x+1,y)
//   t(x,y) = q(x,y) + s(x,y)
//   nb     = (t(x,y-1) + t(x,y+1)) + q(x,y)
//   v'(c)  = (v(c) - out(c)) + nb
// No multiply/add pair is fused (-ffp-contract=off), the division is the IEEE one, and rows
// outside the grid and columns >= W of v and f weigh 0 by select, never by multiplication
// (the pitch padding may hold NaN).
//
// The streaming design is mm_pass_kernel's (mm_kernels.hip): a wave owns a strip of 128
// columns x TH rows, lane l moves columns 2l, 2l+1 as one 16-B load / store, lanes 0 and 63
// also carry the column left / right of the strip, three rows of shares s slide down the
// strip in registers, t of the left / right column comes from the adjacent lanes through
// DPP wave_shr:1 / wave_shl:1, U input rows stay in flight, and rows outside the launch
// get descriptors with num_records = 0, so every iteration issues the same memory
// instructions. What differs: every input row loads v and f (a 128-bit load each plus the
// edge column of each), and the share needs no division where the strip lies at least two
// columns inside the grid and the row has three in-grid rows (s = out * 0.125); the
// division runs on wave-uniform edge rows and strips only. About 9 fp64 operations against
// 24 B per cell (read v, read f, write v'): HBM-bound by a wide margin.
// Attributes outside field_mask are copied through (the pass flips every attribute's
// ping-pong buffers).
#include "mm_inst.hpp"
#include "mm_lane.hpp"

namespace mm {

namespace {

// One input row as this lane sees it: values and rates of its two columns and its edge column.
template <int NA>
struct FRaw {
    double v0[NA], v1[NA], ve[NA];
    double f0[NA], f1[NA], fe[NA];
};

// Processed row: the shares of the three columns and v - out (v itself for an attribute
// that is copied through) of the two own columns.
template <int NA>
struct FRow {
    double s0[NA], s1[NA], se[NA];
    double d0[NA], d1[NA];
};

template <int NA>
__device__ __forceinline__ void fload_row(const PassArgs& A, int r, int rmax, unsigned voff,
                                          unsigned eoff, FRaw<NA>& o) {
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        const bool dif = A.field_mask & (1 << a);  // kernel-uniform
        const __amdgpu_buffer_rsrc_t rs = row_rsrc(A.in[a], r, rmax, A.pitch);
        const dv2 p = __builtin_bit_cast(dv2, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, 0, 0));
        o.v0[a] = p.x;
        o.v1[a] = p.y;
        if (dif) {
            o.ve[a] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rs, eoff, 0, 0));
            const __amdgpu_buffer_rsrc_t rf = row_rsrc(A.field[a], r, rmax, A.pitch);
            const dv2 q = __builtin_bit_cast(dv2, __builtin_amdgcn_raw_buffer_load_b128(rf, voff, 0, 0));
            o.f0[a] = q.x;
            o.f1[a] = q.y;
            o.fe[a] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rf, eoff, 0, 0));
        } else {
            o.ve[a] = o.f0[a] = o.f1[a] = o.fe[a] = 0.0;
        }
    }
}

template <int NA>
__device__ __forceinline__ void fprocess_row(const PassArgs& A, int r, const FRaw<NA>& raw,
                                             bool fast_cols, int sy0, int sy1, int sye,
                                             FRow<NA>& o) {
    const int sx = span3(A.H, A.x_init + r);  // wave-uniform
    const bool fast = sx == 3 && fast_cols;    // cnt == 8 in all three columns
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        if (!(A.field_mask & (1 << a))) {  // copied through
            o.s0[a] = o.s1[a] = o.se[a] = 0.0;
            o.d0[a] = raw.v0[a];
            o.d1[a] = raw.v1[a];
            continue;
        }
        double out0, out1, oute;
        if (fast) {
            out0 = raw.f0[a] * raw.v0[a];
            out1 = raw.f1[a] * raw.v1[a];
            oute = raw.fe[a] * raw.ve[a];
            o.s0[a] = out0 * 0.125;
            o.s1[a] = out1 * 0.125;
            o.se[a] = oute * 0.125;
        } else {
            // (sx == 0: a row outside the grid; sy == 0: a column outside it -- the pitch
            // padding -- or no edge column: the share is 0 by select)
            share_one(raw.v0[a], raw.f0[a], sx && sy0, sx * sy0 - 1, out0, o.s0[a]);
            share_one(raw.v1[a], raw.f1[a], sx && sy1, sx * sy1 - 1, out1, o.s1[a]);
            share_one(raw.ve[a], raw.fe[a], sx && sye, sx * sye - 1, oute, o.se[a]);
        }
        o.d0[a] = raw.v0[a] - out0;
        o.d1[a] = raw.v1[a] - out1;
    }
}

template <int NA, bool REDUCE, int NT>
__device__ __forceinline__ void femit_row(const PassArgs& A, int r, int rmax, unsigned voff,
                                          bool st2, bool st1, const FRow<NA>& P, const FRow<NA>& C,
                                          const FRow<NA>& N, double (&acc)[NA]) {
    const bool live = r <= rmax;  // wave-uniform
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        double w0, w1;
        if (A.field_mask & (1 << a)) {
            const double q0 = P.s0[a] + N.s0[a], q1 = P.s1[a] + N.s1[a], qe = P.se[a] + N.se[a];
            const double t0 = q0 + C.s0[a], t1 = q1 + C.s1[a], te = qe + C.se[a];
            const double left = dpp_from_lower_lane(t1, te);   // t at column y0-1
            const double right = dpp_from_upper_lane(t0, te);  // t at column y0+2
            w0 = C.d0[a] + ((left + t1) + q0);
            w1 = C.d1[a] + ((t0 + right) + q1);
        } else {
            w0 = C.d0[a];
            w1 = C.d1[a];
        }
        dv2 v;
        v.x = w0;
        v.y = w1;
        // lanes past W write the row's padding columns (never read as cells)
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v),
                                               row_rsrc(A.out[a], r, rmax, A.pitch), voff, 0,
                                               (NT & 1) ? 2 : 0);
        if (REDUCE) {
            acc[a] = acc[a] + ((live && st1) ? w0 : 0.0);
            acc[a] = acc[a] + ((live && st2) ? w1 : 0.0);
        }
    }
}

template <int NA>
__device__ __forceinline__ void fcopy_row(FRow<NA>& d, const FRow<NA>& s) {
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        d.s0[a] = s.s0[a];
        d.s1[a] = s.s1[a];
        d.se[a] = s.se[a];
        d.d0[a] = s.d0[a];
        d.d1[a] = s.d1[a];
    }
}

// TH output rows per wave, fully unrolled; the wave mapping and row ranges are
// mm_pass_kernel's (ra0..rb1, th, nstrips, waves_a, waves_total, partials, partial_base), so
// the planner's one-step launches drive it unchanged.
template <int NA, int TH, int U, bool REDUCE, int NT>
__global__ __launch_bounds__(kBlock) void mm_field_kernel(const PassArgs A) {
    static_assert(U <= TH, "prefetch deeper than the row block");
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
    const int strip = (int)(w % A.nstrips);
    const int rb = (int)(w / A.nstrips);
    const int rA = rlo + rb * TH;
    const int rB = min(rA + TH, rhi);  // output rows [rA, rB); input rows [rA-1, rB]

    const long long base = (long long)strip * kStripCols;
    const long long y0 = base + 2 * lane;
    const long long W = A.W;
    // lane 0 carries the column left of the strip, lane 63 the one right of it
    const long long ye = lane == 0 ? base - 1 : (lane == 63 ? base + kStripCols : -1);
    const bool edge_ok = ye >= 0 && ye < W;
    const int sy0 = span3(W, y0), sy1 = span3(W, y0 + 1), sye = edge_ok ? span3(W, ye) : 0;
    const bool fast_cols = base >= 2 && base + kStripCols <= W - 2;  // wave-uniform
    const bool st1 = y0 < W, st2 = y0 + 1 < W;
    const unsigned voff = (unsigned)(y0 * 8);
    const unsigned eoff = edge_ok ? (unsigned)(ye * 8) : kOOB;

    double acc[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) acc[a] = 0.0;

    // Input row rA-1+i is "input i". Inputs 0 and 1 prime the window; input i >= 2 lives in
    // raw[(i-2) % U] and is refilled with input i+U as soon as it is consumed.
    FRaw<NA> first, second, raw[U];
    fload_row<NA>(A, rA - 1, rB, voff, eoff, first);
    fload_row<NA>(A, rA, rB, voff, eoff, second);
#pragma unroll
    for (int k = 0; k < U; ++k) fload_row<NA>(A, rA + 1 + k, rB, voff, eoff, raw[k]);
    FRow<NA> P, C, N;
    fprocess_row<NA>(A, rA - 1, first, fast_cols, sy0, sy1, sye, P);
    fprocess_row<NA>(A, rA, second, fast_cols, sy0, sy1, sye, C);
#pragma unroll
    for (int k = 0; k < TH; ++k) {
        fprocess_row<NA>(A, rA + 1 + k, raw[k % U], fast_cols, sy0, sy1, sye, N);
        if (k + U < TH)  // input k+2+U is still inside this row block
            fload_row<NA>(A, rA + 1 + k + U, rB, voff, eoff, raw[k % U]);
        femit_row<NA, REDUCE, NT>(A, rA + k, rB - 1, voff, st2, st1, P, C, N, acc);
        fcopy_row<NA>(P, C);
        fcopy_row<NA>(C, N);
    }

    if (REDUCE) {
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            const double t = wave_sum(acc[a]);
            if (lane == 0) A.partials[(A.partial_base + wid) * NA + a] = t;
        }
    }
}

template <int NA, int TH, int U, int NT>
hipError_t launch_f(bool reduce, const PassArgs& a, hipStream_t s) {
    const long long blocks = (a.waves_total + kWavesPerBlock - 1) / kWavesPerBlock;
    return launch_inst(reduce ? *inst_of<mm_field_kernel<NA, TH, U, true, NT>, kBlock>()
                              : *inst_of<mm_field_kernel<NA, TH, U, false, NT>, kBlock>(),
                       blocks, a, s);
}

// rows kept in flight per wave (each row: v and f of every attribute); fewer as the
// attributes, and the registers per row, grow
template <int NA>
constexpr int field_prefetch() {
    return NA == 1 ? 8 : (NA == 2 ? 4 : 2);
}

template <int NA>
hipError_t launch_field_na(bool reduce, const PassArgs& a, hipStream_t s, int variant) {
    if (a.th == 1) return launch_f<NA, 1, 1, 0>(reduce, a, s);  // border row of a split pass
    if (a.th != 8) return hipErrorInvalidValue;
    if (NA == 1 && (variant & 1)) return launch_f<1, 8, 8, 1>(reduce, a, s);  // non-temporal stores
    return launch_f<NA, 8, field_prefetch<NA>(), 0>(reduce, a, s);
}

}  // namespace

hipError_t launch_field(int na, bool reduce, const PassArgs& a, hipStream_t s, int variant) {
    if (a.waves_total <= 0) return hipSuccess;
    switch (na) {
        case 1: return launch_field_na<1>(reduce, a, s, variant);
        case 2: return launch_field_na<2>(reduce, a, s, variant);
        case 3: return launch_field_na<3>(reduce, a, s, variant);
        case 4: return launch_field_na<4>(reduce, a, s, variant);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace mm
