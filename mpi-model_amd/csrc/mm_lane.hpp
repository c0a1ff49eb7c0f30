// mm_lane.hpp -- the lane-level primitives every gfx950 kernel of the engine shares: the
// neighbour-count tables, the wave shifts and sums, the buffer-descriptor idioms and the
// transfer chain. They encode the arithmetic contract of oracle/mm_oracle.h once, for the
// one-step kernels (mm_kernels.hip, mm_field.hip) and the K-step kernels (mm_passk.hpp,
// mm_wide.hpp) alike. All __forceinline__: the header adds no code of its own.
#pragma once

#include "mm_internal.hpp"

namespace mm {

namespace {

typedef double dv2 __attribute__((ext_vector_type(2)));
typedef double dv8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr unsigned kOOB = 0x80000000u;  // voffset past any num_records: loads 0, stores dropped

// A neighbour's weight factor 8/cnt in the whole-grid step (oracle/mm_oracle.c c8_of: w =
// u * 8/cnt, u itself for an interior cell, 0 outside the grid -- each neighbour's share
// out/cnt is (r/8) * w): the correctly rounded quotients as constants, no division at run
// time.
__device__ __forceinline__ double c8_of(int cnt) {
    return cnt == 8 ? 1.0
                    : (cnt == 5 ? 8.0 / 5.0
                                : (cnt == 3 ? 8.0 / 3.0
                                            : (cnt == 2 ? 4.0 : (cnt == 1 ? 8.0 : 0.0))));
}

// The own-weight coefficient -(8 + 8/cnt) of the box sum (oracle/mm_oracle.c m_of): -9 for
// an interior cell, 0 for a cell without neighbours (it keeps its value) or outside the grid.
constexpr double kM8 = -9.0;
constexpr double kM5 = -(8.0 + 8.0 / 5.0);
__device__ __forceinline__ double m8_of(int cnt) {
    return cnt == 8 ? kM8
                    : (cnt == 5 ? kM5
                                : (cnt == 3 ? -(8.0 + 8.0 / 3.0)
                                            : (cnt == 2 ? -12.0 : (cnt == 1 ? -16.0 : 0.0))));
}

// Rate-field diffusion (mm_field.hip, mm_fieldk.hpp): the share of one emitter with cnt
// in-grid neighbours (src/Model.hpp:199); in_grid false or cnt == 0: the cell emits
// nothing, by select
__device__ __forceinline__ void share_one(double v, double f, bool in_grid, int cnt, double& out,
                                          double& s) {
    const bool emits = in_grid && cnt > 0;
    out = emits ? f * v : 0.0;
    s = cnt == 8 ? out * 0.125 : (emits ? out / (double)cnt : 0.0);
}

// The two wave shifts by one lane, in two flavours. update_dpp with a tied `old`: the lanes
// without a source lane (0 / 63) keep `old` -- the one-step kernels, whose edge lanes carry
// the column beside the strip there.
__device__ __forceinline__ double dpp_from_lower_lane(double src, double old) {
    // lane i <- lane i-1 (wave_shr:1); lane 0 keeps `old`
    const long long s = __double_as_longlong(src), o = __double_as_longlong(old);
    const int lo = __builtin_amdgcn_update_dpp((int)o, (int)s, 0x138, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(o >> 32), (int)(s >> 32), 0x138, 0xf, 0xf, false);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

__device__ __forceinline__ double dpp_from_upper_lane(double src, double old) {
    // lane i <- lane i+1 (wave_shl:1); lane 63 keeps `old`
    const long long s = __double_as_longlong(src), o = __double_as_longlong(old);
    const int lo = __builtin_amdgcn_update_dpp((int)o, (int)s, 0x130, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(o >> 32), (int)(s >> 32), 0x130, 0xf, 0xf, false);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// mov_dpp (the K-step kernels) has no tied "old" operand, so the result can land in a fresh
// register without first copying the source; lanes without a source lane read 0
// (bound_ctrl) -- only the halo lanes at the wave's edges, whose results are discarded.
__device__ __forceinline__ double dpp_lower(double src) {
    // lane i <- lane i-1 (wave_shr:1)
    const long long s = __double_as_longlong(src);
    const int lo = __builtin_amdgcn_mov_dpp((int)s, 0x138, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_mov_dpp((int)(s >> 32), 0x138, 0xf, 0xf, true);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

__device__ __forceinline__ double dpp_upper(double src) {
    // lane i <- lane i+1 (wave_shl:1)
    const long long s = __double_as_longlong(src);
    const int lo = __builtin_amdgcn_mov_dpp((int)s, 0x130, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_mov_dpp((int)(s >> 32), 0x130, 0xf, 0xf, true);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// The same two shifts through the LDS crossbar (ds_bpermute_b32: no LDS memory, the DS
// pipe instead of the VALU). A DPP shift of a double is two VALU moves, 4 of the 18 VALU
// instructions of a level-row of two columns; ds_bpermute moves them to the otherwise idle
// DS pipe. `addr` = 4 * source lane (wraps around the wave: the halo lanes get garbage
// instead of 0, and their results are discarded either way).
__device__ __forceinline__ double lds_shift(double src, int addr) {
    const long long s = __double_as_longlong(src);
    const int lo = __builtin_amdgcn_ds_bpermute(addr, (int)s);
    const int hi = __builtin_amdgcn_ds_bpermute(addr, (int)(s >> 32));
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

__device__ __forceinline__ double wave_sum(double v) {
    // fixed butterfly: every lane ends with the same, order-independent-of-timing value
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}

// Buffer descriptor of local row r of one attribute buffer. Rows outside [0, rmax] get
// num_records = 0: their loads return 0 and their stores are dropped with no memory
// traffic, so every loop iteration issues the same memory instructions (the compiler
// can then keep counted vmcnt waits across the loop instead of draining it).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t row_rsrc(const double* buf, int r, int rmax,
                                                           long long pitch) {
    const bool ok = r <= rmax;
    const double* p = buf + (long long)(ok ? r : 0) * pitch;
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(p), 0,
                                             ok ? (int)(pitch * 8) : 0, 0x00020000);
}

// Transfers of a chain, in declared order, on one cell's attribute values: out = r*u_a;
// u_a -= out; u_b += out (b < 0: the outflow leaves the system). a and b are wave-uniform
// kernel arguments, and chain entries are read with compile-time indices only, so they are
// scalar loads of the kernel arguments that the compiler hoists out of the row loop (a
// runtime index into the by-value PassArgs turns into per-row global loads and vmcnt(0)
// waits that drain the row prefetch). The values sit in one 8-element register vector for
// the chain -- at that width LLVM indexes it with s_set_gpr_idx (two v_mov per access)
// instead of a select over every attribute per operand (36 v_cndmask per transfer and
// column) -- and a pad slot takes the outflows that leave the system.
#ifndef MM_CHAIN_CAP
#define MM_CHAIN_CAP kMaxChain  // transfers a chain may hold (tuning: fewer unrolled slots)
#endif
template <int NA>
__device__ __forceinline__ void chain_k(double (&u)[NA], int n, const signed char* ta,
                                        const signed char* tb, const double* tr) {
    static_assert(NA < 8, "one pad slot");
    dv8 v;
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = k < NA ? u[k] : 0.0;
#pragma unroll
    for (int t = 0; t < MM_CHAIN_CAP; ++t) {
        if (t >= n) break;  // wave-uniform
        const int a = ta[t];
        const int b = tb[t] >= 0 ? tb[t] : 7;
        const double out = tr[t] * v[a];
        v[a] = v[a] - out;
        v[b] = v[b] + out;
    }
#pragma unroll
    for (int k = 0; k < NA; ++k) u[k] = v[k];
}

}  // namespace

}  // namespace mm
