// mm_closed.hip -- gfx950 kernel of the closed rate-field diffusion (MM_FLOW_DIFFUSE_CLOSED):
// the rate-field diffusion of mm_field.hip on an irregular domain. A cell is OPEN when it is
// inside the grid and its rate f is not zero (+0 and -0 are both walls); everything else is a
// wall, which takes no share, gives none and keeps its bits.
//
// Arithmetic contract (include/mpimodel.h; tests/closed_model.py restates it in numpy). For
// the in-grid cell c = (x, y) with cnt(c) OPEN Moore neighbours (0..8):
//   out(c) = f(c) * v(c)              if c is open and cnt(c) > 0, else 0       (by select)
//   s(c)   = out(c) * 0.125           if cnt(c) == 8
//            out(c) / (double)cnt(c)  if 1 <= cnt(c) <= 7
//            0                        otherwise (walls, cnt == 0, outside the grid; by select)
//   q(x,y) = s(x-1,y) + s(x+1,y)
//   t(x,y) = q(x,y) + s(x,y)
//   nb     = (t(x,y-1) + t(x,y+1)) + q(x,y)
//   v'(c)  = (v(c) - out(c)) + nb     if c is open;  v(c), bit for bit, if c is a wall
// Operation for operation mm_field_kernel's order (-ffp-contract=off, the IEEE division):
// where f != 0 on the whole grid the two agree bit for bit. A wall is a wall by select, never
// by multiplication: it may hold NaN, an infinity or -0, and so may the pitch padding.
//
// The streaming design is mm_field_kernel's: a wave owns a strip of 128 columns x TH rows,
// lane l moves columns 2l, 2l+1 as one 16-B load / store, lanes 0 and 63 also carry the
// column beside the strip, three rows of shares slide down the strip in registers, t of the
// neighbouring columns comes through DPP wave_shr:1 / wave_shl:1, U rows stay in flight, and
// rows outside the launch get descriptors with num_records = 0. Same PassArgs row ranges,
// wave map and partials, so the planner's one-step launches drive it unchanged.
//
// What is new is the count. cnt(c) is no matter of geometry: output row x needs the shares
// of rows x-1..x+1, whose counts need the openness of rows x-2..x+2 and of one column more
// on each side than the shares. So f runs one row ahead of v (TH + 4 rows of f against
// TH + 2 of v per block), lanes 0 / 63 load f of the TWO columns beside the strip (one
// aligned 16-B load) and each row of f becomes four openness bits per lane (own columns,
// edge column, the column behind it); columns >= W and rows outside the grid are closed by
// select on the global index. The bits of a row add up to column triples (the +-1 column
// through the DPP shifts), packed a byte each for the three columns a lane carries; the box
// count of a row is the sum of three rows' triples (one 32-bit add: no byte exceeds 9) and
// cnt = box - own bit. The window holds the triples of three rows and the bits of one, on
// top of the two rows still in flight: five rows of openness. No extra HBM stream: 24 B per
// cell of the diffusing attribute, 16 B per attribute copied through.
// Whether the division can be skipped is decided per row from the data: a box byte of 9
// means "open with eight open neighbours", and a wave ballot tells whether that holds in
// every column the wave carries (s = out * 0.125, no select); a second ballot skips rows in
// which nothing emits; every other row runs the general body (share_one: IEEE division,
// walls and cnt == 0 by select).
// A pass holds exactly one closed diffusion (A.field_mask has one bit); the engine's other
// attributes are copied through (the pass flips every attribute's ping-pong buffers).
#include "mm_inst.hpp"
#include "mm_lane.hpp"

namespace mm {

namespace {

// the wave shifts of mm_lane.hpp on a 32-bit word: lanes without a source lane keep `old`
__device__ __forceinline__ int dpp32_from_lower_lane(int src, int old) {
    return __builtin_amdgcn_update_dpp(old, src, 0x138, 0xf, 0xf, false);  // wave_shr:1
}
__device__ __forceinline__ int dpp32_from_upper_lane(int src, int old) {
    return __builtin_amdgcn_update_dpp(old, src, 0x130, 0xf, 0xf, false);  // wave_shl:1
}

// What a lane knows of its place: byte offsets of its loads, which of its columns are
// inside the grid, and whether it carries an edge column.
struct CLane {
    unsigned voff;   // own two columns
    unsigned eoff;   // edge column (kOOB: none, or outside the grid)
    unsigned poff;   // the aligned pair of columns beside the strip that holds the edge column
    bool st1, st2;   // own columns inside the grid
    bool edge, far;  // edge column / the column behind it inside the grid
    bool l0, edge_lane;
};

// One row of rates as loaded: own columns and the pair beside the strip.
struct CFRaw {
    double f0, f1, pa, pb;
};
// One row of values as loaded.
struct CVRaw {
    double v0, v1, ve;
};
// A row of rates turned into openness: bit 0 / 1 own columns, 2 edge column, 3 the column
// behind it; `tri` the open cells among columns y-1..y+1, one byte per column (own, own,
// edge); the rates the share still needs.
struct CORow {
    int ob, tri;
    double f0, f1, fe;
};
// Processed row: shares of the three columns, v - out of the own columns (v itself for a
// wall, by select), the openness bits.
struct CSRow {
    double s0, s1, se, d0, d1;
    int ob;
};

__device__ __forceinline__ void cf_load(const double* fin, int r, int rmax, long long pitch,
                                        const CLane& L, CFRaw& o) {
    const __amdgpu_buffer_rsrc_t rf = row_rsrc(fin, r, rmax, pitch);
    const dv2 q = __builtin_bit_cast(dv2, __builtin_amdgcn_raw_buffer_load_b128(rf, L.voff, 0, 0));
    const dv2 p = __builtin_bit_cast(dv2, __builtin_amdgcn_raw_buffer_load_b128(rf, L.poff, 0, 0));
    o.f0 = q.x, o.f1 = q.y, o.pa = p.x, o.pb = p.y;
}

__device__ __forceinline__ void cv_load(const double* vin, int r, int rmax, long long pitch,
                                        const CLane& L, CVRaw& o) {
    const __amdgpu_buffer_rsrc_t rs = row_rsrc(vin, r, rmax, pitch);
    const dv2 p = __builtin_bit_cast(dv2, __builtin_amdgcn_raw_buffer_load_b128(rs, L.voff, 0, 0));
    o.v0 = p.x, o.v1 = p.y;
    o.ve = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rs, L.eoff, 0, 0));
}

// Openness of local row r from its rates. A row outside the grid is closed (wave-uniform
// select on the global row), a column outside it by the lane's flags.
__device__ __forceinline__ void copen_row(const PassArgs& A, int r, const CLane& L,
                                          const CFRaw& raw, CORow& o) {
    const long long gx = A.x_init + r;
    const bool rin = gx >= 0 && gx < A.H;
    // lane 0: the pair is columns base-2, base-1; lane 63: base+128, base+129
    const double fe = L.l0 ? raw.pb : raw.pa, ff = L.l0 ? raw.pa : raw.pb;
    const int b0 = (rin && L.st1 && raw.f0 != 0.0) ? 1 : 0;
    const int b1 = (rin && L.st2 && raw.f1 != 0.0) ? 1 : 0;
    const int be = (rin && L.edge && fe != 0.0) ? 1 : 0;
    const int bf = (rin && L.far && ff != 0.0) ? 1 : 0;
    const int ob = b0 | b1 << 1 | be << 2 | bf << 3;
    // bit 1 of the lower lane's word is column y0-1 (lane 0: its edge bit, moved there);
    // bit 0 of the upper lane's is column y0+2 (lane 63: its edge bit)
    const int left = (dpp32_from_lower_lane(ob, ob >> 1) >> 1) & 1;
    const int right = dpp32_from_upper_lane(ob, ob >> 2) & 1;
    const int h0 = left + b0 + b1, h1 = b0 + b1 + right;
    const int he = L.l0 ? bf + be + b0 : b1 + be + bf;  // (lanes 1..62: never used)
    o.ob = ob;
    o.tri = h0 | h1 << 8 | he << 16;
    o.f0 = raw.f0, o.f1 = raw.f1, o.fe = fe;
}

// Shares of one row: `box` = open cells of the 3 x 3 box of each column (a byte each), the
// sum of the triples of the rows above, of this row and below.
__device__ __forceinline__ void cshare_row(const CLane& L, int tri_up, const CORow& O, int tri_dn,
                                           const CVRaw& raw, CSRow& o) {
    const int box = tri_up + O.tri + tri_dn;
    const int b0 = O.ob & 1, b1 = (O.ob >> 1) & 1, be = (O.ob >> 2) & 1;
    // a box of 9: the cell is open and so are its eight neighbours
    const bool all8 = (box & 0xffff) == 0x0909 && (!L.edge_lane || (box >> 16) == 9);
    const bool emits = ((box & 0xff) > 1 && b0) || (((box >> 8) & 0xff) > 1 && b1) ||
                       (L.edge_lane && (box >> 16) > 1 && be);
    o.ob = O.ob;
    if (__builtin_amdgcn_ballot_w64(all8) == ~0ull) {  // wave-uniform: no division, no select
        const double out0 = O.f0 * raw.v0, out1 = O.f1 * raw.v1, oute = O.fe * raw.ve;
        o.s0 = out0 * 0.125;
        o.s1 = out1 * 0.125;
        o.se = oute * 0.125;
        o.d0 = raw.v0 - out0;
        o.d1 = raw.v1 - out1;
    } else if (__builtin_amdgcn_ballot_w64(emits) == 0ull) {  // walls and lone cells only
        o.s0 = o.s1 = o.se = 0.0;
        o.d0 = b0 ? raw.v0 - 0.0 : raw.v0;
        o.d1 = b1 ? raw.v1 - 0.0 : raw.v1;
    } else {
        double out0, out1, oute;
        share_one(raw.v0, O.f0, b0, (box & 0xff) - b0, out0, o.s0);
        share_one(raw.v1, O.f1, b1, ((box >> 8) & 0xff) - b1, out1, o.s1);
        share_one(raw.ve, O.fe, be, ((box >> 16) & 0xff) - be, oute, o.se);
        o.d0 = b0 ? raw.v0 - out0 : raw.v0;
        o.d1 = b1 ? raw.v1 - out1 : raw.v1;
    }
}

template <bool REDUCE, int NT>
__device__ __forceinline__ void cemit_row(double* vout, int r, int rmax, long long pitch,
                                          const CLane& L, const CSRow& P, const CSRow& C,
                                          const CSRow& N, double& acc) {
    const double q0 = P.s0 + N.s0, q1 = P.s1 + N.s1, qe = P.se + N.se;
    const double t0 = q0 + C.s0, t1 = q1 + C.s1, te = qe + C.se;
    const double left = dpp_from_lower_lane(t1, te);   // t at column y0-1
    const double right = dpp_from_upper_lane(t0, te);  // t at column y0+2
    const double w0 = (C.ob & 1) ? C.d0 + ((left + t1) + q0) : C.d0;
    const double w1 = (C.ob & 2) ? C.d1 + ((t0 + right) + q1) : C.d1;
    dv2 v;
    v.x = w0;
    v.y = w1;
    // lanes past W write the row's padding columns (never read as cells)
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v),
                                           row_rsrc(vout, r, rmax, pitch), L.voff, 0,
                                           (NT & 1) ? 2 : 0);
    if (REDUCE) {
        const bool live = r <= rmax;  // wave-uniform
        acc = acc + ((live && L.st1) ? w0 : 0.0);
        acc = acc + ((live && L.st2) ? w1 : 0.0);
    }
}

// TH output rows per wave, fully unrolled. Row rA-2+j is "input j": rates of inputs
// 0..TH+3, values of inputs 1..TH+2. Rates of inputs 0..3 and values of inputs 1, 2 prime the
// window; rate input j >= 4 lives in fr[(j-4) % U], value input j >= 3 in vr[(j-3) % U], each
// refilled as soon as it is consumed. NC = NA - 1 attributes are copied through, U rows of
// them in flight.
template <int NA, int TH, int U, bool REDUCE, int NT>
__global__ __launch_bounds__(kBlock) void mm_closed_kernel(const PassArgs A) {
    static_assert(U <= TH, "prefetch deeper than the row block");
    constexpr int NC = NA - 1, NCA = NC ? NC : 1;
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
    const int rB = min(rA + TH, rhi);  // output rows [rA, rB); v rows [rA-1, rB], f [rA-2, rB+1]

    // the closed attribute and the copied ones (kernel-uniform; the kernel arguments are read
    // with compile-time indices only)
    const int ca = NA == 1 ? 0 : __builtin_ctz((unsigned)A.field_mask);
    const double* vin = A.in[0];
    const double* fin = A.field[0];
    double* vout = A.out[0];
    const double* cin[NCA];
    double* cout[NCA];
#pragma unroll
    for (int a = 1; a < NA; ++a)
        if (ca == a) {
            vin = A.in[a];
            fin = A.field[a];
            vout = A.out[a];
        }
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        cin[j] = j < ca ? A.in[j] : A.in[j + 1];
        cout[j] = j < ca ? A.out[j] : A.out[j + 1];
    }

    const long long base = (long long)strip * kStripCols;
    const long long y0 = base + 2 * lane;
    const long long W = A.W, pitch = A.pitch;
    CLane L;
    L.l0 = lane == 0;
    L.edge_lane = lane == 0 || lane == 63;
    // lane 0 carries columns base-2, base-1, lane 63 columns base+128, base+129
    const long long ye = L.l0 ? base - 1 : (lane == 63 ? base + kStripCols : -1);
    const long long yf = L.l0 ? base - 2 : (lane == 63 ? base + kStripCols + 1 : -1);
    L.edge = ye >= 0 && ye < W;
    L.far = yf >= 0 && yf < W;
    L.st1 = y0 < W;
    L.st2 = y0 + 1 < W;
    L.voff = (unsigned)(y0 * 8);
    L.eoff = L.edge ? (unsigned)(ye * 8) : kOOB;
    // both columns of the pair lie inside the row's pitch: base is a multiple of 128 and W at
    // most the pitch, so base - 2 >= 126 and base + 129 < pitch wherever the edge column is
    // inside the grid
    L.poff = L.edge ? (unsigned)((L.l0 ? base - 2 : base + kStripCols) * 8) : kOOB;

    double acc = 0.0, acc_c[NCA];
#pragma unroll
    for (int j = 0; j < NCA; ++j) acc_c[j] = 0.0;

    CFRaw fp[4], fr[U];
    CVRaw vp[2], vr[U];
    dv2 cr[U][NCA];
#pragma unroll
    for (int j = 0; j < 4; ++j) cf_load(fin, rA - 2 + j, rB + 1, pitch, L, fp[j]);
    cv_load(vin, rA - 1, rB, pitch, L, vp[0]);
    cv_load(vin, rA, rB, pitch, L, vp[1]);
#pragma unroll
    for (int k = 0; k < U; ++k) {
        cf_load(fin, rA + 2 + k, rB + 1, pitch, L, fr[k]);
        cv_load(vin, rA + 1 + k, rB, pitch, L, vr[k]);
#pragma unroll
        for (int j = 0; j < NC; ++j)
            cr[k][j] = __builtin_bit_cast(
                dv2, __builtin_amdgcn_raw_buffer_load_b128(row_rsrc(cin[j], rA + k, rB - 1, pitch),
                                                           L.voff, 0, 0));
    }

    CORow Oa, Ob, On;
    CSRow P, C, N;
    {
        CORow o0, o1;
        copen_row(A, rA - 2, L, fp[0], o0);
        copen_row(A, rA - 1, L, fp[1], o1);
        copen_row(A, rA, L, fp[2], Oa);
        copen_row(A, rA + 1, L, fp[3], Ob);
        cshare_row(L, o0.tri, o1, Oa.tri, vp[0], P);
        cshare_row(L, o1.tri, Oa, Ob.tri, vp[1], C);
    }
#pragma unroll
    for (int k = 0; k < TH; ++k) {
        copen_row(A, rA + 2 + k, L, fr[k % U], On);  // rate input k+4
        if (k + U < TH)                              // rate input k+4+U <= TH+3
            cf_load(fin, rA + 2 + k + U, rB + 1, pitch, L, fr[k % U]);
        cshare_row(L, Oa.tri, Ob, On.tri, vr[k % U], N);  // value input k+3, row rA+1+k
        if (k + U < TH)                                   // value input k+3+U <= TH+2
            cv_load(vin, rA + 1 + k + U, rB, pitch, L, vr[k % U]);
        cemit_row<REDUCE, NT>(vout, rA + k, rB - 1, pitch, L, P, C, N, acc);
#pragma unroll
        for (int j = 0; j < NC; ++j) {  // the attributes copied through, row rA+k
            const dv2 c = cr[k % U][j];
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, c),
                                                   row_rsrc(cout[j], rA + k, rB - 1, pitch),
                                                   L.voff, 0, 0);
            if (REDUCE) {
                const bool live = rA + k <= rB - 1;
                acc_c[j] = acc_c[j] + ((live && L.st1) ? c.x : 0.0);
                acc_c[j] = acc_c[j] + ((live && L.st2) ? c.y : 0.0);
            }
            if (k + U < TH)
                cr[k % U][j] = __builtin_bit_cast(
                    dv2, __builtin_amdgcn_raw_buffer_load_b128(
                             row_rsrc(cin[j], rA + k + U, rB - 1, pitch), L.voff, 0, 0));
        }
        P = C;
        C = N;
        Oa = Ob;
        Ob = On;
    }

    if (REDUCE) {
        double* part = A.partials + (A.partial_base + wid) * NA;
        const double t = wave_sum(acc);
        if (lane == 0) part[ca] = t;
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const double tc = wave_sum(acc_c[j]);
            if (lane == 0) part[j < ca ? j : j + 1] = tc;
        }
    }
}

template <int NA, int TH, int U, int NT>
hipError_t launch_c(bool reduce, const PassArgs& a, hipStream_t s) {
    const long long blocks = (a.waves_total + kWavesPerBlock - 1) / kWavesPerBlock;
    return launch_inst(reduce ? *inst_of<mm_closed_kernel<NA, TH, U, true, NT>, kBlock>()
                              : *inst_of<mm_closed_kernel<NA, TH, U, false, NT>, kBlock>(),
                       blocks, a, s);
}

// rows kept in flight per wave: a row of v, a row of f one row ahead of it, and a row of
// every attribute copied through
template <int NA>
constexpr int closed_prefetch() {
    return NA == 1 ? 6 : 4;
}

template <int NA>
hipError_t launch_closed_na(bool reduce, const PassArgs& a, hipStream_t s, int variant) {
    if (a.th == 1) return launch_c<NA, 1, 1, 0>(reduce, a, s);  // border row of a split pass
    if (a.th != 8) return hipErrorInvalidValue;
    if (NA == 1 && (variant & 1))  // non-temporal stores
        return launch_c<1, 8, closed_prefetch<1>(), 1>(reduce, a, s);
    return launch_c<NA, 8, closed_prefetch<NA>(), 0>(reduce, a, s);
}

}  // namespace

hipError_t launch_closed(int na, bool reduce, const PassArgs& a, hipStream_t s, int variant) {
    if (a.waves_total <= 0) return hipSuccess;
    // exactly one closed diffusion per pass, of an attribute of the engine, with a field
    if (__builtin_popcount((unsigned)a.field_mask) != 1 || a.field_mask >= (1 << na))
        return hipErrorInvalidValue;
    if (!a.field[__builtin_ctz((unsigned)a.field_mask)]) return hipErrorInvalidValue;
    switch (na) {
        case 1: return launch_closed_na<1>(reduce, a, s, variant);
        case 2: return launch_closed_na<2>(reduce, a, s, variant);
        case 3: return launch_closed_na<3>(reduce, a, s, variant);
        case 4: return launch_closed_na<4>(reduce, a, s, variant);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace mm
