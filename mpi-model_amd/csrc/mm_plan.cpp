// mm_plan.cpp -- the host-only planner (mm_plan.hpp).
#include "mm_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace mm {

namespace {

constexpr double kAny = 1e300;

// name, 'i' integer (lo <= v <= hi) or 'd' real (lo < v <= hi), range, what a value in
// range sets; the defaults are Knobs' initialisers. Order matters where a row reads an
// earlier one (MM_STEPS_PER_PASS after MM_WIDE).
struct KnobRow {
    const char* name;
    char type;
    double lo, hi;
    void (*set)(Knobs&, double);
};

const KnobRow kKnobRows[] = {
    {"MM_GRAPH", 'i', -kAny, kAny, [](Knobs& k, double v) { k.graphs_ok = v != 0; }},
    {"MM_GRAPH_MIN_STEPS", 'i', 1, 256, [](Knobs& k, double v) { k.graph_min = (long long)v; }},
    {"MM_GRAPH_MAX_LAUNCHES", 'i', 1, 4096, [](Knobs& k, double v) { k.graph_max = (long long)v; }},
    // Rows per wave of the one-step kernel (a compile-time row block: 8, 16 or 32). Short
    // blocks give the most waves in flight, which is what the memory system wants
    // (tools/sweep.py, profiles/r01): 8 by default
    {"MM_ROWS_PER_WAVE", 'i', 8, 32, [](Knobs& k, double v) { if (v == 8 || v == 16 || v == 32) k.th = (int)v; }},
    {"MM_FUSE", 'i', -kAny, kAny, [](Knobs& k, double v) { k.passk = k.passk && v != 0; }},
    {"MM_PASSK", 'i', -kAny, kAny, [](Knobs& k, double v) { k.passk = k.passk && v != 0; }},
    {"MM_WIDE", 'i', -kAny, kAny, [](Knobs& k, double v) { k.wide = v != 0 ? 1 : 0; }},
    {"MM_STEPS_PER_PASS", 'i', 1, kAny,
     [](Knobs& k, double d) {
         const int v = (int)std::min(d, 1e9);
         if (v <= kMaxSteps || (k.wide != 0 && (wide_has(v, 4, 1) || wide_has(v, 2, 4)))) k.kpass = v;
         k.kpass_multi = std::min(v, 2);
     }},
    {"MM_PASS_PLAN", 'i', -kAny, kAny, [](Knobs& k, double v) { k.plan = v != 0; }},
    {"MM_SEG_WAVES", 'd', 0, kAny, [](Knobs& k, double v) { k.seg_waves = v; }},
    {"MM_SEG_EDGE", 'd', 0, 1, [](Knobs& k, double v) { k.seg_edge = v; }},
    {"MM_XCD_REMAP", 'i', -kAny, kAny, [](Knobs& k, double v) { k.xcd = v != 0; }},
    {"MM_BORDER_SEGMENTS", 'i', -kAny, kAny, [](Knobs& k, double v) { k.border_segments = v != 0; }},
    {"MM_CHAIN_RING", 'i', -kAny, kAny, [](Knobs& k, double v) { k.ring_ok = v != 0; }},
    {"MM_SYNC_SPIN", 'i', -kAny, kAny, [](Knobs& k, double v) { k.sync_spin = v != 0; }},
    {"MM_SELF_HALO", 'i', -kAny, kAny, [](Knobs& k, double v) { k.self_halo = v != 0; }},
    {"MM_KERNEL_VARIANT", 'i', 0, kAny, [](Knobs& k, double v) { k.variant = (int)std::min(v, 1e9); }},
    {"MM_FIELD_STEPS", 'i', 0, kFieldMaxSteps, [](Knobs& k, double v) { k.field_steps = (int)v; }},
    {"MM_FIELD_HALO", 'i', 1, kFieldMaxSteps, [](Knobs& k, double v) { k.field_halo = (int)v; }},
    {"MM_CLOSED_STEPS", 'i', 0, kAny,
     [](Knobs& k, double v) { k.closed_steps = (int)std::min(v, (double)kClosedMaxSteps); }},
    {"MM_CLOSED_HALO", 'i', 2, kClosedMaxSteps + 1, [](Knobs& k, double v) { k.closed_halo = (int)v; }},
    {"MM_WIDE_COLS", 'i', 4, kWide6Cols, [](Knobs& k, double v) { if (v != 5) k.wide_cols = (int)v; }},
};

}  // namespace

Knobs read_knobs(const std::function<const char*(const char*)>& get) {
    Knobs k;
    for (const KnobRow& r : kKnobRows) {
        const char* s = get(r.name);
        if (!s) continue;
        const double v = r.type == 'i' ? (double)std::atoll(s) : std::atof(s);
        if ((r.type == 'i' ? v >= r.lo : v > r.lo) && v <= r.hi) r.set(k, v);
    }
    return k;
}

namespace {

constexpr double kWideCells = 268435456.0;  // 2^28: 16384^2, 8192 x 32768 and up
// Below 2^25 cells (4096^2 and down) one K = 8 pass of the level-split kernel beats
// mm_passk_kernel's K = 7 / 8: its 4 waves share a segment's pipeline fill, so segments
// are 2.7x longer for the same number of resident waves (1000 steps of 4096^2: 1513-1585
// vs 1410-1443 GCUPS; one pass per step at 1024^2 / 2048^2: 4.54 / 6.39 vs 6.22 / 6.69 us,
// profiles/r03/c2graph); 8192^2 favours mm_passk_kernel K = 7 (32.4 vs 35.0 us).
constexpr double kWideSmallCells = 33554432.0;
constexpr int kWideSmallAuto = 8;
// the K = 20 planner's slabs (forced MM_WIDE=1 plans every slab that way)
// Slabs of 2^27 - 2^28 cells (the 4096 x 32768 slabs of an 8-GPU c3 run) also take the
// K = 20 planner. Round 4 kept mm_passk_kernel there without a halo (2050 vs ~1920 GCUPS,
// profiles/r04/midslab); since the box-sum step the level-split kernel runs the split
// 4096 x 32768 slab at 2532 GCUPS against 1194-1272 for mm_passk_kernel's 7 + 7 + 6 without
// one (20 steps, profiles/r06/self20, profiles/r06/selfhalo).
constexpr double kWideSplitCells = 134217728.0;  // 2^27
constexpr int kWideAuto = 20;      // auto steps per pass of the wide kernel, one attribute
constexpr int kWideAutoMulti = 8;  // several attributes

// sized by the chain's thinnest slab (rank-invariant, like every plan input)
double slab_cells(const PlanIn& in) { return (double)in.min_rows * (double)in.W; }

// Columns per lane of the wide kernel: 4 for one attribute, 2 for several.
int wcols(const PlanIn& in) { return in.n_attr > 1 ? 2 : 4; }

bool wide_big(const PlanIn& in) {
    return in.knobs.wide > 0 || slab_cells(in) >= kWideCells ||
           (in.knobs.wide < 0 && in.n_attr == 1 && slab_cells(in) >= kWideSplitCells);
}

bool wide_on(const PlanIn& in) {
    // auto: several attributes always (K = 8 instead of mm_passk_kernel's 2); one attribute
    // on slabs of >= kWideSplitCells or < kWideSmallCells cells
    return in.knobs.wide > 0 ||
           (in.knobs.wide < 0 && (in.n_attr > 1 || wide_big(in) || slab_cells(in) < kWideSmallCells));
}

// The level-split kernel runs a pass of k steps: one of its instances, MM_WIDE on; four
// attributes: a pass with at least one diffusion (the instances diffuse 1..4).
bool use_wide(const PlanIn& in, int k) {
    return wide_on(in) && passk_ok(in) && wide_has(k, wcols(in), in.n_attr) &&
           (in.n_attr == 1 || in.diffuse_mask != 0);
}

long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }

// Steps per K-step pass: the configured K, capped so that a depth-K halo never reaches
// past the thinnest slab of the chain (every rank sends K owned rows each way).
int passk_steps(const PlanIn& in) {
    // one attribute, auto: K = 8 on slabs of >= 2^27 cells, else 7 -- the fastest K per
    // step of the round-2 sweeps (profiles/r02/sweep_k_*.log, profiles/r02c/sweep_*x32768:
    // 32768^2, 16384^2 and the 8192- and 4096-row slabs of 32768 columns favour 8, 4096^2
    // with its short segments 7; K <= 4 leaves the VALU idle behind the HBM stream)
    // wide (mm_wide_kernel): auto K = kWideAuto
    // (wide on a small slab: kWideSmallAuto passes, no planner)
    const Knobs& kn = in.knobs;
    const bool wide1 = wide_on(in) && in.n_attr == 1;
    const int kauto = wide1 ? (wide_big(in) ? kWideAuto : kWideSmallAuto)
                            : (slab_cells(in) >= kWideSplitCells ? 8 : 7);
    int k1 = kn.kpass > 0 ? kn.kpass : kauto;
    if (!wide1) k1 = std::min(k1, kMaxSteps);  // mm_passk_kernel's K
    int k = in.n_attr == 1 ? k1 : std::min(kn.kpass_multi, passk_max_steps(in.n_attr));
    // several attributes, wide kernel: its K (auto kWideAutoMulti), or mm_passk_kernel's
    if (in.n_attr > 1 && wide_on(in) && passk_ok(in)) {
        k = kn.kpass > 0 ? kn.kpass : kWideAutoMulti;
        if (!wide_has(k, 2, in.n_attr)) k = std::min(k, passk_max_steps(in.n_attr));
    }
    if (in.nranks > 1) k = (int)std::min<long long>(k, in.min_rows);
    return std::max(1, k);
}

// Modelled time of one K-step pass of a large one-attribute slab, relative to the K = 8
// pass: the HBM stream of the grid (`kStream`: the K <= 7 passes, which the stream
// bounds), or the VALU work of K levels over the strips' 128 - 4*ceil(K/2) output
// columns, whichever is longer (K >= 8 are VALU-bound: 32768^2 on one box, K = 8 / 9 /
// 10: 3437 / 3884 / 4326 us, profiles/r02b/k9k10/edge_*; K = 7 0.93 of K = 8,
// profiles/r02b/segwaves).
double pass_cost(int k) {
    constexpr double kStream = 0.93;
    constexpr double kValuPerLevel = 112.0 / (8.0 * 128.0);  // K = 8 -> 1.0
    const double useful = (double)passk_out_cols(k) / (double)kStripCols;
    return std::max(kStream, kValuPerLevel * (double)k / useful);
}

// A pass of k steps has a kernel: the wide one (use_wide) or mm_passk_kernel (k <= 10).
bool pass_len_ok(const PlanIn& in, long long k) {
    return k >= 1 && (k <= passk_max_steps(in.n_attr) || use_wide(in, (int)k));
}

// Modelled time of one k-step pass on a large slab with the wide kernel on, in ms at
// 32768^2: mm_passk_kernel K <= 7 stream-bound at ~3.5 ms, K = 8 / 9 / 10 at 3.66 / 4.14 /
// 4.62 (profiles/r02b); mm_wide_kernel K = 4 / 8 at 3.69 / 3.68 (profiles/r03/kernel_table)
// and K = 12 / 16 / 20 at 0.778 / 1 / 1.236 of the K = 16 pass (one box,
// profiles/r03/xcd2/kernel_table.log: 5120 / 6578 / 8128 us; K = 20 with ascending levels).
double wide_plan_cost(const PlanIn& in, int k) {
    if (use_wide(in, k)) {
        switch (k) {
            case 4: return 3.69;
            case 8: return 3.68;
            case 12: return 4.84;
            case 16: return 6.22;
            default: return 7.69;
        }
    }
    if (k <= 7) return 3.50;
    return k == 8 ? 3.66 : (k == 9 ? 4.14 : 4.62);
}

// Steps of the first pass of the cheapest plan of n steps (wide on, K auto): a dynamic
// program over the pass lengths both kernels have (capped by the chain's thinnest slab).
// Runs longer than kDpMax steps start with a pass of the best per-step length (K = 20).
int wide_plan_first(const PlanIn& in, long long n, int kcap) {
    constexpr int kDpMax = 256;
    if (n > kDpMax) return std::min(kWideAuto, kcap);
    double cost[kMaxWide + 1];
    for (int k = 1; k <= std::min(kcap, kMaxWide); ++k) cost[k] = pass_len_ok(in, k) ? wide_plan_cost(in, k) : -1.0;
    std::vector<double> best((size_t)n + 1, 1e300);
    std::vector<int> first((size_t)n + 1, 1);
    best[0] = 0.0;
    for (long long m = 1; m <= n; ++m)
        for (int k = 1; k <= std::min<long long>(m, kcap); ++k) {
            if (cost[k] < 0.0) continue;
            const double c = cost[k] + best[(size_t)(m - k)];
            if (c < best[(size_t)m] * (1.0 - 1e-9)) {
                best[(size_t)m] = c;
                first[(size_t)m] = k;
            }
        }
    return first[(size_t)n];
}

// The rate kinds whose passes may fuse K steps: the kernel of such a pass, the PlanIn field
// that holds its K, and the geometry of its k-step pass (mm_geom.hpp).
struct RateKind {
    Kernel kernel;
    bool closed;  // steps: closed_k of a closed program, field_k of any other
    int (*out_cols)(int k);
    long long (*max_rows)(int k, long long pitch);
    int steps(const PlanIn& in) const { return closed ? in.closed_k : in.field_k; }
};
const RateKind kRateKinds[] = {{kFieldK, false, passk_out_cols, fieldk_max_rows},
                               {kClosedK, true, closedk_out_cols, closedk_max_rows}};

// The kind whose passes the program fuses, K = steps(in) >= 2 steps each (the engine set
// field_k / closed_k); nullptr: the program fuses no rate kind.
const RateKind* fused_kind(const PlanIn& in) {
    for (const RateKind& r : kRateKinds)
        if (r.steps(in) >= 2 && in.closed == r.closed) return &r;
    return nullptr;
}

const RateKind* rate_kind_of(Kernel kernel) {
    for (const RateKind& r : kRateKinds)
        if (r.kernel == kernel) return &r;
    return nullptr;
}

// Edge-strip segment length / interior segment length of a k-step pass (MM_SEG_EDGE
// overrides). mm_passk_kernel: the two edge strips run the general body, several times
// slower per row than the branch-free one, and at K >= 8 it spills; their segments are cut
// shorter so they end with the rest (profiles/r02b/k9k10/edge_*: K = 10 at 0.5 takes 1.5x
// the pass time of 0.1; profiles/r02_end/edge/sweep_*: on slabs of >= 2^26 cells K = 6..8
// at 0.3 are 1-3 % faster than at 0.5 at 16384^2 and within 0.2 % at 32768^2; the short
// segments of smaller slabs keep 0.5). mm_wide_kernel: full-length segments for one
// attribute (the EDGE / GEN bodies cost little more than the interior's since round 5:
// c2 / c3 +0.5-1.5 %, c4 and the split slabs within +-1 %), half length for four (their
// per-column GEN body: C5 -10 % at full length; profiles/r05/edge).
double seg_edge_of(const PlanIn& in, Kernel kernel, int k) {
    if (in.knobs.seg_edge > 0.0) return in.knobs.seg_edge;
    // mm_fieldk_kernel: the general body adds a short division per edge cell and keeps the
    // levels interleaved; full-length edge segments until a measurement says otherwise.
    // mm_closedk_kernel chooses its body from the data, row by row, in every strip alike:
    // full-length edge segments, not measured otherwise
    if (rate_kind_of(kernel)) return 1.0;
    if (kernel == kWide) return in.n_attr == 1 ? 1.0 : 0.5;
    if (k >= 10) return 0.1;
    if (k == 9) return 0.2;
    return (double)in.h * (double)in.W >= 67108864.0 ? 0.3 : 0.5;
}

long long waves_for(long long nstrips, long long n, int th) { return n <= 0 ? 0 : nstrips * ceil_div(n, th); }

// MM_FIELD_STEPS unset: K = kFieldAutoSteps on slabs of at least kFieldAutoCells cells
// (the table of tools/bench_field.py: the built K of the best time per step
// at 8192^2, and the smallest measured size at which it beat the one-step pass in all three
// rounds). Never below 2^16 cells: small field grids keep one step per pass.
constexpr int kFieldAutoSteps = 4;
constexpr double kFieldAutoCells = 4194304.0;  // 2048^2
static_assert(kFieldAutoCells >= 65536.0 && kFieldAutoSteps <= kFieldMaxSteps, "auto rule");
// The same rule on a slab with a halo (field_k_for), by the cells of the chain's thinnest
// slab: the smallest measured slab at which the split K = 4 pass beat the split one-step pass
// of the same run (the table of tools/bench_field.py --self-halo).
constexpr double kFieldAutoCellsHalo = 4194304.0;
static_assert(kFieldAutoCellsHalo >= kFieldAutoCells, "a halo never lowers the auto threshold");

}  // namespace

int field_steps_for(const PlanIn& in) {
    const int k = in.knobs.field_steps;
    if (!in.knobs.passk || k == 1 || in.pitch <= 0 || fieldk_max_rows(kFieldMaxSteps, in.pitch) < 64)
        return 0;
    if (k >= 2) return std::min(k, kFieldMaxSteps);
    return (double)in.h * (double)in.W >= kFieldAutoCells ? kFieldAutoSteps : 0;
}

int field_k_for(const PlanIn& in, bool halo) {
    if (in.closed) return 0;  // mm_closed_kernel runs one step per pass
    if (!halo) return field_steps_for(in);
    // sized by the chain's thinnest slab, like every plan input of a chain
    PlanIn thin = in;
    thin.h = in.min_rows;
    int k = field_steps_for(thin);
    if (in.knobs.field_steps == 0 && slab_cells(in) < kFieldAutoCellsHalo) k = 0;
    k = (int)std::min<long long>(std::min(k, in.knobs.field_halo), in.min_rows);
    return k >= 2 ? k : 0;
}

int closed_field_promise(const Knobs& knobs) { return std::max(knobs.field_halo, knobs.closed_halo); }

int closed_k_for(const PlanIn& in, bool halo) {
    int k = std::min(in.knobs.closed_steps, kClosedMaxSteps);
    if (!in.closed || !in.knobs.passk || k < 2 || in.pitch <= 0 ||
        closedk_max_rows(kClosedMaxSteps, in.pitch) < 64)
        return 0;
    // a k-step pass reads k + 1 ghost rows of the field and sends k owned rows each way: the
    // knobs and the chain's thinnest slab, never the rows uploaded or this slab's own.
    // MM_CLOSED_HALO alone opts in: MM_FIELD_HALO keeps changing no plan of a closed program
    if (halo) k = (int)std::min<long long>(std::min(k, in.knobs.closed_halo - 1), in.min_rows);
    return k >= 2 ? k : 0;
}

bool kstep_ok(const PlanIn& in) { return fused_kind(in) || passk_ok(in); }

bool passk_ok(const PlanIn& in) {
    if (!in.knobs.passk || in.n_passes != 1 || in.field) return false;
    if (passk_max_rows(kMaxSteps, in.pitch) < 64) return false;
    if (in.n_attr == 1) return in.diffuse_mask == 1 && !in.chains;
    return true;
}

bool wide6_on(const PlanIn& in, int k, bool red) {
    // planned from the fused instance's occupancy: a caller that has no such instance
    // (slots6 unset) plans every pass at 4 columns
    if (!in.slots6 || in.knobs.wide_cols == 4 || k != kMaxWide || red || in.n_attr != 1 || in.split ||
        in.nranks != 1 || in.x_init != 0 || in.h != in.H || !use_wide(in, k))
        return false;
    if (wide6_cols(in.W).strips == 0) return false;
    return in.knobs.wide_cols == kWide6Cols || slab_cells(in) >= kWideSplitCells;
}

namespace {

// kernel_for but for the fused six-column pass
KernelChoice kernel4_for(const PlanIn& in, int k) {
    // a rate-field program in K-step passes: a pass of one step stays on mm_field_kernel, and
    // a closed program's on mm_closed_kernel
    const RateKind* r = fused_kind(in);
    if (r && k >= 2) return {r->kernel, 2, ceil_div(in.W, r->out_cols(k))};
    if (!passk_ok(in)) return {kOneStep, 1, 0};  // one mm_pass_kernel launch per pass of the step
    if (use_wide(in, k)) return {kWide, wcols(in), ceil_div(in.W, wide_out_cols(k, wcols(in)))};
    return {kPassK, 2, ceil_div(in.W, passk_out_cols(k))};
}

}  // namespace

KernelChoice kernel_for(const PlanIn& in, int k, bool red) {
    if (wide6_on(in, k, red)) {  // the strips between the bands: first, six-column, right
        const Wide6Cols c = wide6_cols(in.W);
        return {kWide, kWide6Cols, 1 + c.strips + c.rstrips};
    }
    return kernel4_for(in, k);
}

int steps_per_launch(const PlanIn& in) {
    if (const RateKind* r = fused_kind(in)) return r->steps(in);
    return passk_ok(in) ? passk_steps(in) : 1;
}

// Steps of the next K-step pass when n steps remain: ceil(n / K) passes of balanced
// length (20 steps at K = 8: 7 + 7 + 6, not 8 + 8 + 4), where K is the auto or configured
// steps per pass. On a large one-attribute slab with K auto, the planner also considers
// fewer, longer passes (up to kMaxSteps, capped by the chain's thinnest slab) and takes
// the plan of least modelled time: 20 steps run as 10 + 10, a long run stays at K = 8
// (1000 steps: 125 passes).
int next_pass_len(const PlanIn& in, long long n) {
    // a rate-field program, closed or not: ceil(n / K) balanced passes (7 steps at K = 4: 4 + 3)
    if (const RateKind* r = fused_kind(in)) return (int)ceil_div(n, ceil_div(n, r->steps(in)));
    if (!passk_ok(in)) return 1;
    const Knobs& kn = in.knobs;
    const int kp = passk_steps(in);
    if (wide_on(in)) {
        if (in.n_attr == 1 && kn.kpass == 0 && kn.plan && wide_big(in)) {
            int cap = kMaxWide;
            if (in.nranks > 1) cap = (int)std::min<long long>(cap, in.min_rows);
            return wide_plan_first(in, n, cap);
        }
        // several attributes or a configured K: passes of K while n >= K, a shorter run in
        // one pass when a kernel has that length, else the longest length a kernel has
        long long k = std::min<long long>(n, kp);
        while (k > 1 && !pass_len_ok(in, k)) --k;
        return (int)std::max<long long>(1, k);
    }
    long long best_p = ceil_div(n, kp);
    // the planner's slabs: >= 2^28 cells in >= 256 strips. With fewer strips the two edge
    // strips (the general body, which spills at K >= 9) weigh more and deep passes lose:
    // 16384^2, 20 steps: 10 + 10 2.85 ms vs 7 + 7 + 6 2.61 ms; 32768 columns at 8192 and
    // 32768 rows: 10 + 10 wins by 7 % (profiles/r02_end/k10tune, profiles/r02c).
    const bool big = slab_cells(in) >= kWideCells && ceil_div(in.W, passk_out_cols(kMaxSteps)) >= 256;
    if (kn.plan && kn.kpass == 0 && in.n_attr == 1 && big && n > kp) {
        long long kx = passk_max_steps(1);
        if (in.nranks > 1) kx = std::min<long long>(kx, in.min_rows);
        double best = 1e300;
        const long long p_max = best_p;
        for (long long p = ceil_div(n, kx); p <= p_max; ++p) {
            const long long q = n / p, r = n % p;  // r passes of q + 1 steps, p - r of q
            const double t = (double)r * pass_cost((int)q + 1) + (double)(p - r) * pass_cost((int)q);
            if (t < best * (1.0 - 1e-9)) {
                best = t;
                best_p = p;
            }
        }
    }
    return (int)ceil_div(n, best_p);
}

std::vector<int> pass_lengths(const PlanIn& in, long long n) {
    std::vector<int> lens;
    for (long long s = 0; s < n; s += lens.back()) lens.push_back(next_pass_len(in, n - s));
    return lens;
}

// Waves of a segment-scheduled range of n rows over ns strips (mm_passk.hpp seg_map).
long long seg_wave_count(long long n, long long ns, long long r, long long re) {
    if (n <= 0) return 0;
    if (ns < 3) return ns * ceil_div(n, re);
    return 2 * ceil_div(n, re) + (ns - 2) * ceil_div(n, r);
}

// Segment plan of n rows of a k-step pass: r rows per interior-strip segment, re per
// edge-strip segment (seg_edge_of x r), the smallest r for which every wave (mm_wide_kernel:
// every workgroup, one per strip segment) fits seg_waves x the chip's resident slots (the
// kernel's occupancy x CUs).
Segments segments(const PlanIn& in, Kernel kernel, int k, int slots, long long n, long long ns) {
    const RateKind* rate = rate_kind_of(kernel);
    const long long maxr =
        std::max<long long>(16, rate ? rate->max_rows(k, in.pitch) : passk_max_rows(k, in.pitch));
    const double edge = seg_edge_of(in, kernel, k);
    const double units = ns < 3 ? (double)ns / edge : (double)(ns - 2) + 2.0 / edge;
    // even segment lengths: with an even first row (x_init and lo even, as every bench
    // slab) no segment pays the odd-start shift of the row-paired kernels (one extra row)
    auto even_rows = [&](long long rr) { return std::min(maxr & ~1LL, rr + (rr & 1)); };
    auto re_of = [&](long long rr) {
        return even_rows(std::min(maxr, std::max<long long>(8, (long long)((double)rr * edge))));
    };
    auto plan = [&](double sw) {
        const long long want = std::max<long long>(1, (long long)(sw * in.ncu * slots));
        long long r = (long long)std::ceil((double)std::max<long long>(n, 1) * units / (double)want);
        r = std::min(std::max<long long>(r, 16), maxr);
        while (r < maxr && seg_wave_count(n, ns, r, re_of(r)) > want) r += std::max<long long>(1, r / 64);
        return even_rows(std::min(r, maxr));
    };
    long long r;
    if (in.knobs.seg_waves > 0.0) {
        r = plan(in.knobs.seg_waves);
    } else if (kernel == kWide) {
        // 4, 3, 2, 1 segment waves per slot while segments are shorter than 20 K rows -- a
        // segment pays 3K - 1 pipeline iterations and 2K extra input rows, 15 % of a 318-row
        // segment at K = 16 (4096 x 32768, profiles/r03/kernel_table): the 4096 x 32768
        // split slab of an 8-GPU c3 run takes 3 (460-row segments; 2 gave 683: kernel
        // 1000-1022 vs 1069-1082 us, 200 steps +2.9 %, profiles/r05/sw3); the other bench
        // shapes keep their plans (c2 ends at 1, 32768^2 / 16384^2 / 8192-row slabs at 4)
        double sw = 4.0;
        r = plan(sw);
        while (sw > 1.0 && r < 20LL * k) {
            sw -= 1.0;
            r = plan(sw);
        }
    } else {
        // 4 waves per slot while segments stay >= 256 rows (large slabs: the waves that
        // finish last are shorter), else 2 (short segments pay 2K extra input rows each) --
        // profiles/r02b/segwaves: 32768^2 K = 7/8 and 16384^2 K = 6..8 run 3-5 % faster at 4
        // than at 2, 4096^2 K = 7 12 % slower.
        r = plan(4.0);
        if (r < 256) r = plan(2.0);
    }
    const long long re = re_of(r);
    return {(int)r, (int)re, seg_wave_count(n, ns, r, re)};
}

Segments segments(const PlanIn& in, int k, bool red, long long lo, long long hi) {
    const KernelChoice kc = kernel4_for(in, k);  // (the six-column pass: wide6_launch)
    return segments(in, kc.kernel, k, std::max(1, in.slots(kc.kernel, k, red)), hi - lo, kc.strips);
}

namespace {

int slots6_of(const PlanIn& in, int k) { return std::max(1, in.slots6(k)); }

// The fused six-column pass of the whole grid (wide6_on). Columns: wide6_cols. Rows: the
// interior strips run the FAST body from their first pipeline iteration to their last, so
// every row a level of them reads -- rows top - k .. bot + k - 1 -- lies in [2, H - 3]; top and
// bot even (the interior segments then all start at even rows: no odd-start shift). A grid too
// low for interior rows is all band. One segment length for the frame's strips between the
// bands and the six-column strips: segments() of all of them at the fused instance's occupancy.
Launch wide6_launch(const PlanIn& in, int k) {
    const Wide6Cols c = wide6_cols(in.W);
    const long long h = in.h;
    Launch l;
    l.lo = 0, l.hi = h, l.seg = 1;
    l.nstrips = (int)ceil_div(in.W, wide_out_cols(k, 4));
    Wide6& w = l.c6;
    w.col = c.col, w.rcol = c.rcol, w.strips = c.strips, w.rstrips = c.rstrips;
    w.top = (int)std::min<long long>(k + 2, h);
    w.bot = (int)std::max<long long>(w.top, (h - k - 2) & ~1LL);
    w.band0 = l.nstrips;
    w.band1 = w.band0 + (w.bot < h ? l.nstrips : 0);
    w.frame = w.band1;
    l.waves_total = w.band1;
    const long long n = w.bot - w.top;
    if (n > 0) {
        const long long ns = 1 + c.rstrips + c.strips;
        const Segments s = segments(in, kWide, k, slots6_of(in, k), n, ns);
        l.th = l.th_edge = w.th = s.th;
        const long long per = ceil_div(n, s.th);
        w.frame = w.band1 + (1 + c.rstrips) * per;
        l.waves_total = w.frame + c.strips * per;
    } else {
        l.th = l.th_edge = w.th = 2;  // (no block between the bands)
    }
    l.waves_a = l.waves_total;
    return l;
}

}  // namespace

PassLaunches pass_launches(const PlanIn& in, int k, bool red) {
    PassLaunches p{};
    p.kern = kernel_for(in, k, red);
    if (p.kern.cols == kWide6Cols && p.kern.kernel == kWide) {
        p.depth = k;
        p.interior = wide6_launch(in, k);
        p.total = p.interior.waves_total;
        return p;
    }
    const Kernel kernel = p.kern.kernel;
    const long long h = in.h;
    const int ns = kernel == kOneStep ? (int)(in.pitch / kStripCols) : (int)p.kern.strips;
    p.depth = kernel == kOneStep ? 1 : k;
    p.split = in.split && h >= 2 * p.depth + 1;  // else: slab too thin, one launch after the exchange
    auto blocks = [&](long long lo, long long hi, long long lo2, long long hi2, int th) {
        Launch l;
        l.lo = lo, l.hi = hi, l.lo2 = lo2, l.hi2 = hi2, l.th = th, l.nstrips = ns;
        l.waves_a = waves_for(ns, hi - lo, th);
        l.waves_total = l.waves_a + waves_for(ns, hi2 - lo2, th);
        return l;
    };
    auto segs = [&](long long lo, long long hi) {
        const Segments s = segments(in, k, red, lo, hi);
        Launch l;
        l.lo = lo, l.hi = hi, l.seg = 1, l.th = s.th, l.th_edge = s.th_edge, l.nstrips = ns;
        l.waves_a = l.waves_total = s.count;
        return l;
    };
    // T border rows a side read the exchanged ghost rows and run after the exchange. The
    // wide kernel by default runs them as the top and bottom segments of every strip at the
    // slab plan's full segment length (what the unsplit plan would run there), the rest of
    // the plan beside the exchange: a K-row border segment paid the K = 20 pipeline fill
    // (~94 iterations) for 20 rows beside the interior (MM_BORDER_SEGMENTS=0).
    long long T = p.split ? p.depth : 0;
    if (p.split && kernel == kWide && in.knobs.border_segments)
        T = std::min<long long>(std::max<long long>(segs(0, h).th, p.depth), h / 2);
    p.interior = kernel == kOneStep ? blocks(T, h - T, 0, 0, in.knobs.th) : segs(T, h - T);
    if (kernel == kPassK) p.interior.xcd_remap = in.knobs.xcd;
    if (p.split) {
        if (kernel == kWide) {  // one T-row segment per strip and side
            p.border = blocks(0, T, h - T, h, (int)T);
            p.border.seg = 1, p.border.th_edge = (int)T;
            p.border.waves_a = seg_wave_count(T, ns, T, T);
            p.border.waves_total = 2 * p.border.waves_a;
        } else {  // short row blocks, the launch is latency-bound
            p.border = blocks(0, T, h - T, h, kernel == kOneStep ? 1 : kBorderRows);
        }
        p.border.partial_base = p.interior.waves_total;
    }
    p.total = p.interior.waves_total + p.border.waves_total;
    return p;
}

SlabPlan slab_plan(const PlanIn& in) {
    const int spl = steps_per_launch(in);
    const KernelChoice kc = kernel_for(in, spl);
    if (kc.kernel == kOneStep)
        return {kOneStep, spl, in.knobs.th, waves_for(in.pitch / kStripCols, in.h, in.knobs.th), 0};
    if (kc.cols == kWide6Cols && kc.kernel == kWide) {  // the fused six-column pass's own plan
        const Launch l = wide6_launch(in, spl);
        return {kWide, spl, l.th, l.waves_total * kWide20Waves, slots6_of(in, spl) * kWide20Waves};
    }
    const Segments s = segments(in, spl, false, 0, in.h);
    const int per =kc.kernel == kWide ? wide_waves_per_block(spl, kc.cols, in.n_attr, in.ring) : 1;
    return {kc.kernel, spl, s.th, s.count * per, std::max(1, in.slots(kc.kernel, spl, false)) * per};
}

// Graph plan of a run of nsteps steps: `per` steps per replayed graph (0: run eagerly).
// A graph holds a whole number of K-step passes, an even number of buffer flips (so the
// captured pointers are valid again) and of reduction periods (so the phase is the same at
// every replay).
long long graph_per(const PlanIn& in, long long nsteps, long long reduce_every, bool any) {
    auto gcd = [](long long a, long long b) {
        while (b) {
            const long long t = a % b;
            a = b;
            b = t;
        }
        return a;
    };
    const long long unit = steps_per_launch(in);
    const long long flips = kstep_ok(in) ? 1 : (long long)in.n_passes;  // per unit: one pass
    long long len = unit * ((flips % 2) ? 2 : 1);
    if (reduce_every > 0) len = len / gcd(len, reduce_every) * reduce_every;
    if (len > 256 || nsteps < len || (!in.knobs.graphs_ok && !any)) return 0;
    long long per = len;
    while (per < in.knobs.graph_min && per * 2 <= nsteps) per *= 2;
    // a short run that is not a whole number of graphs becomes one graph (its passes
    // balanced, pass_lengths), instead of graphs plus an eager tail; keyed by the buffer
    // parity like every graph, so an odd number of flips is fine
    if (nsteps % per != 0 && nsteps <= 64 * unit) per = nsteps;
    // fewer, longer graphs: consecutive graph launches start ~9 us apart on the GPU, the
    // kernels inside one graph back to back (c2, 16-step graphs: 62 such gaps in 1000
    // steps, 5 % of the run, profiles/r04/final/prof_c2_k8). So the longest whole number of
    // base blocks (the pass length and the reduce period, so every graph starts at the
    // same phase) that divides the run, up to graph_max step kernels
    const long long base = reduce_every > 0 ? unit / gcd(unit, reduce_every) * reduce_every : unit;
    if (nsteps % base == 0) {
        const long long m = nsteps / base, per_block = base / unit * flips;  // kernels per block
        for (long long d = std::min(m, in.knobs.graph_max / per_block); d * base > per; --d)
            if (m % d == 0) {
                per = d * base;
                break;
            }
    }
    return per;
}

long long partials_need(const PlanIn& in) {
    // doubles: one-step kernel, 128-column strips x 8-row blocks with kMaxAttr sums per
    // wave (+ 1-row border blocks); mm_passk_kernel, segments of >= 8 rows (edge strips)
    // plus 4-row border blocks (depth <= kGhost rows on each side) with K x NA sums per
    // wave: K <= kMaxSteps for one attribute, K <= 2 for up to kMaxAttr; mm_fieldk_kernel,
    // segments of >= 8 rows over no more strips than these plus, split, one 4-row border
    // block per strip and side, K <= kFieldMaxSteps sums per wave; mm_closedk_kernel, segments
    // of >= 8 rows over fewer strips still (closedk_out_cols) plus, split, its 4-row border
    // blocks, K <= kClosedMaxSteps sums per wave
    const long long ns1 = in.pitch / kStripCols;
    const long long need = (waves_for(ns1, in.h, 8) + 2 * waves_for(ns1, 2, 1) + 16) * kMaxAttr;
    const long long ns = ceil_div(in.W, passk_out_cols(kMaxSteps));
    const long long border = 2 * ceil_div(kGhost, kBorderRows) + 2;
    return std::max(need, (ns * ((in.h + 7) / 8 + border) + 16) * std::max(kMaxWide, 8 * kMaxAttr));
}

// non-temporal stores pay once the two buffers outgrow the 256 MiB Infinity Cache
// (profiles/r01 sweeps); MM_KERNEL_VARIANT overrides
int kernel_variant(const PlanIn& in) {
    if (in.knobs.variant >= 0) return in.knobs.variant;
    return 2.0 * 8.0 * (double)in.pitch * (double)in.h * in.n_attr > 256.0 * 1048576.0 ? 1 : 0;
}

}  // namespace mm
