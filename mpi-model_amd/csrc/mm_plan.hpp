// mm_plan.hpp -- what a run does, decided from the slab's shape and the tuning variables:
// which kernel runs a pass of K steps, how many steps each pass takes, how a pass's rows
// are cut into segments and launches, how many steps a replayed graph holds. Plain
// arithmetic: no HIP, no engine; mm_engine.hip launches what this describes, and
// tests/test_plan.py checks it without a GPU. Every rank of a chain must plan the same
// passes (or the K-row exchanges would not pair up), so nothing here reads the rank or
// this slab's own rows where the chain's thinnest slab (min_rows) is meant.
#pragma once

#include <functional>
#include <vector>

#include "mm_geom.hpp"

namespace mm {

// The MM_* tuning variables (include/mpimodel.h lists them), parsed by read_knobs alone.
struct Knobs {
    bool graphs_ok = true;      // MM_GRAPH=0 runs steps eagerly
    long long graph_min = 16;   // steps a replayed graph holds at least (MM_GRAPH_MIN_STEPS)
    long long graph_max = 128;  // step kernels a graph holds at most (MM_GRAPH_MAX_LAUNCHES)
    int th = 8;                 // rows per wave, one-step kernel (MM_ROWS_PER_WAVE: 8, 16, 32)
    bool passk = true;       // mm_passk_kernel for one-pass programs (MM_PASSK=0: one step per pass)
    int wide = -1;           // mm_wide_kernel for one-diffusion programs where K allows
                             // (MM_WIDE=0/1; -1 auto: slabs of >= kWideCells cells)
    int kpass = 0;           // steps per pass, one attribute (MM_STEPS_PER_PASS, 1..kMaxSteps,
                             // with MM_WIDE also the wide kernel's K; 0: auto)
    int kpass_multi = 2;     // steps per pass, several attributes (MM_STEPS_PER_PASS, 1..2)
    bool plan = true;        // pass-length planner (MM_PASS_PLAN=0: balanced passes of K)
    double seg_waves = 0.0;  // segment waves per resident wave slot (MM_SEG_WAVES; 0: auto)
    double seg_edge = 0.0;   // edge-strip segment length / interior length (MM_SEG_EDGE; 0: auto)
    bool border_segments = true;  // wide split passes: full-length border segments (MM_BORDER_SEGMENTS)
    int xcd = 0;             // XCD-contiguous block order (MM_XCD_REMAP, mm_passk_kernel)
    bool ring_ok = true;     // the ring instance for C5-shaped chains (MM_CHAIN_RING=0: off)
    bool sync_spin = true;   // mm_synchronize polls its streams before the blocking wait
                             // (MM_SYNC_SPIN=0: the blocking wait alone)
    bool self_halo = false;  // MM_SELF_HALO: one RCCL rank exchanges border rows with itself
    int variant = -1;        // kernel tuning variant (MM_KERNEL_VARIANT; -1: by buffer size)
    int field_steps = 0;     // steps per rate-field pass (MM_FIELD_STEPS: 1 one step per pass,
                             // 2..kFieldMaxSteps that K on mm_fieldk_kernel; 0: auto)
    int field_halo = 1;      // valid ghost rows of every rate field on each side that has a
                             // neighbour, the caller's promise (MM_FIELD_HALO, 1..kFieldMaxSteps):
                             // bounds the K of a rate-field pass on a slab with a halo
    int closed_steps = 0;    // steps per closed rate-field pass (MM_CLOSED_STEPS: 0 or 1 one step
                             // per pass, 2..kClosedMaxSteps that K on mm_closedk_kernel; no
                             // auto rule)
    int closed_halo = 0;     // valid ghost rows of the rate field of a closed diffusion on each
                             // side that has a neighbour, the caller's promise (MM_CLOSED_HALO,
                             // 2..kClosedMaxSteps + 1; 0: unset): a K-step closed pass on a slab
                             // with a halo reads K + 1 such rows, one more than MM_FIELD_HALO
                             // reaches, and bounds its K by this knob alone; the one-step closed
                             // pass's promise of 2 rows is max(field_halo, closed_halo)
    int wide_cols = 0;       // MM_WIDE_COLS: 6 the fused six-column K = 20 pass wherever its
                             // shape allows (wide6_on), 4 never; 0 auto: slabs of >= 2^27 cells
};
// `get` is std::getenv or a stand-in for it.
Knobs read_knobs(const std::function<const char*(const char*)>& get);

enum Kernel { kOneStep = 0, kPassK = 2, kWide = 3, kFieldK = 4, kClosedK = 5 };  // mm_info.kernel's numbers

struct PlanIn {
    long long H = 0, W = 0, h = 0, x_init = 0;
    int nranks = 1;
    long long min_rows = 0;  // thinnest slab of the chain: bounds the halo depth
    long long pitch = 0;
    int n_attr = 1;
    bool split = false;      // interior / border split (RCCL or host halo)
    // the program's shape: passes per step and, of a one-pass program, what its pass holds
    int n_passes = 0;
    int diffuse_mask = 0;
    bool chains = false;     // pre- or post-chain transfers
    bool ring = false;       // the ring instance runs its K = 8 passes (waves per workgroup)
    bool field = false;      // some pass is a rate-field pass (mm_field_kernel): one step per pass
    bool closed = false;     // some pass is a closed rate-field pass (mm_closed_kernel): field is
                             // set too, and the program stays at one step per pass, halo depth
                             // 1, whatever MM_FIELD_STEPS / MM_FIELD_HALO say (field_k_for: 0),
                             // unless closed_k says otherwise
    int field_k = 0;         // >= 2: the program is one rate-field diffusion of one attribute,
                             // and its passes fuse up to this many steps on mm_fieldk_kernel
                             // (the engine sets field_k_for; 0: off)
    int closed_k = 0;        // >= 2: the program is one closed rate-field diffusion of one
                             // attribute, and its passes fuse up to this many steps on
                             // mm_closedk_kernel (the engine sets closed_k_for; 0: off)
    Knobs knobs;
    int ncu = 0;             // compute units of the device
    // resident wave (kPassK, kFieldK, kClosedK) or workgroup (kWide) slots per CU of the instance that runs a
    // pass of k steps, with the step sums or without: the one plan input the device gives
    std::function<int(Kernel, int k, bool red)> slots;
    // workgroup slots per CU of the fused six-column instance of k steps (mm_wide6_kernel);
    // unset: the caller has no such instance, and every pass plans at 4 columns
    std::function<int(int k)> slots6;
};

struct KernelChoice {
    Kernel kernel;
    int cols;          // columns per lane
    long long strips;  // column strips of a pass (kOneStep: 0, mm_pass_kernel's own)
};

struct Segments {
    int th, th_edge;   // rows per interior-strip and per edge-strip segment
    long long count;   // waves (kPassK, kFieldK, kClosedK) or workgroups (kWide)
};

// The fused six-column pass (mm_wide.hpp mm_wide6_kernel), one launch of rows [lo, hi) = the
// whole grid. Frame, at 4 columns per lane, dispatched first: the band rows [lo, top) and
// [bot, hi) of every column (Launch::nstrips strips), and between the bands the strip of the
// grid's first column and the rstrips strips from column rcol on (the grid's last column
// among them, whatever W % 6 is) in segments of Launch::th rows. Interior: `strips` strips of
// wide_out_cols(k, 6) columns from column col on at 6 columns per lane, rows [top, bot) in
// segments of th rows; every row and column any level of them reads is an interior cell.
// Blocks [0, band0) the top band, [band0, band1) the bottom band, [band1, frame) the frame
// between the bands, [frame, Launch::waves_total) the interior. strips == 0: not such a pass.
struct Wide6 {
    int top = 0, bot = 0, col = 0, rcol = 0, strips = 0, rstrips = 0, th = 0;
    long long band0 = 0, band1 = 0, frame = 0;
};

// One kernel launch: rows [lo, hi) and [lo2, hi2) of the slab, as mm::PassArgs wants them.
struct Launch {
    long long lo = 0, hi = 0, lo2 = 0, hi2 = 0;
    int seg = 0, th = 0, th_edge = 0, xcd_remap = 0, nstrips = 0;
    long long waves_a = 0, waves_total = 0, partial_base = 0;
    Wide6 c6;
};

// One pass: the interior launch on the compute stream and, when split, the border launch
// (the rows that read exchanged ghost rows) on the comm stream.
struct PassLaunches {
    KernelChoice kern;
    int depth;        // halo rows the pass reads on each side
    bool split;
    Launch interior, border;
    long long total;  // partials units of the whole pass
};

// Can the program run on mm_passk_kernel / mm_wide_kernel? One pass per step (one attribute: a single
// diffusion; several: diffusions and transfer chains), no rate-field pass, and buffer offsets
// below 2^31.
bool passk_ok(const PlanIn& in);
// Steps per pass of a program that may run on mm_fieldk_kernel (one attribute, exactly one
// rate-field diffusion -- the engine checks that) on a slab of in.h rows: MM_FIELD_STEPS, or the
// auto rule by the slab's cells; 0 where it stays one step per pass (also with MM_PASSK=0).
int field_steps_for(const PlanIn& in);
// PlanIn::field_k of such a program. Without a halo: field_steps_for. With one (a chain, or
// one slab with a halo mode): min(field_steps_for of the chain's thinnest slab,
// MM_FIELD_HALO, min_rows) -- a K-step pass reads K ghost rows of the rate field, which the
// engine never exchanges and the caller promises; under 2: 0. A program with a closed
// diffusion (in.closed): 0.
int field_k_for(const PlanIn& in, bool halo);
// PlanIn::closed_k of a program that may run on mm_closedk_kernel (one attribute, exactly one
// closed diffusion -- the engine checks that). Without a halo: min(MM_CLOSED_STEPS,
// kClosedMaxSteps). With one (a chain, any halo mode, MM_SELF_HALO): min(that,
// MM_CLOSED_HALO - 1, min_rows) -- a K-step pass reads K + 1 ghost rows of the rate field,
// which the engine never exchanges and the caller promises, and sends K owned rows each way;
// MM_FIELD_HALO changes no plan of a closed program, as before MM_CLOSED_HALO existed.
// Under 2: 0 (one step per pass), as with the knob unset, 0 or 1, under MM_PASSK=0 and where
// closedk_max_rows < 64. No auto rule. Reads the knobs, never the rows uploaded.
int closed_k_for(const PlanIn& in, bool halo);
// Ghost rows of the rate field the caller promised a closed diffusion on every side with a
// neighbour: max(MM_FIELD_HALO, MM_CLOSED_HALO). The one-step closed pass needs 2 (the engine's
// check; no plan reads this).
int closed_field_promise(const Knobs& knobs);
// A run advances in K-step passes of the program's only pass: passk_ok, field_k >= 2 or
// closed_k >= 2.
bool kstep_ok(const PlanIn& in);
// red: the pass sums some of its steps (only the choice of the six-column pass depends on it)
KernelChoice kernel_for(const PlanIn& in, int k, bool red = false);
// The fused six-column pass runs a k-step pass: MM_WIDE_COLS not 4, one attribute on the wide
// kernel, k = 20, an unsplit pass of the whole grid (no halo), no sums, W wide enough for one
// six-column strip between the frame's parts (wide6_cols) and, unless MM_WIDE_COLS=6, a slab
// of >= 2^27 cells.
bool wide6_on(const PlanIn& in, int k, bool red);
// Steps one kernel pass advances: K with the K-step kernels, 1 otherwise. Also the ghost
// rows one exchange must fill.
int steps_per_launch(const PlanIn& in);
int next_pass_len(const PlanIn& in, long long n);
std::vector<int> pass_lengths(const PlanIn& in, long long n);
long long seg_wave_count(long long n, long long ns, long long r, long long re);
// Segment plan of n rows over ns strips with `slots` resident slots per CU.
Segments segments(const PlanIn& in, Kernel kernel, int k, int slots, long long n, long long ns);
Segments segments(const PlanIn& in, int k, bool red, long long lo, long long hi);
PassLaunches pass_launches(const PlanIn& in, int k, bool red);
// What mm_engine_info reports: the whole-slab plan of one pass of steps_per_launch steps,
// in waves (a wide workgroup: wide_waves_per_block waves).
struct SlabPlan {
    Kernel kernel;
    int steps_per_launch, rows_per_wave;
    long long waves_per_pass;
    int seg_waves_per_cu;
};
SlabPlan slab_plan(const PlanIn& in);
long long graph_per(const PlanIn& in, long long nsteps, long long reduce_every, bool any = false);
// Doubles of the partials buffer: room for every pass_launches(k, red).total.
long long partials_need(const PlanIn& in);
int kernel_variant(const PlanIn& in);

}  // namespace mm
