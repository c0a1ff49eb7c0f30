// mm_engine.hip -- the host engine behind include/mpimodel.h (C ABI).
//
// One engine = one row slab of the global grid on one GPU:
//   * device memory: per attribute two (h + 2*kGhost) x pitch fp64 buffers (Jacobi
//     ping-pong) with kGhost ghost rows above and below, pitch a multiple of 128;
//   * a one-pass flow program runs K steps per kernel pass (mm_passk_kernel, temporal
//     blocking: 16/K B of HBM traffic per cell-update); other programs run one step
//     per pass (mm_pass_kernel; mm_field_kernel for a rate-field pass, whose per-cell rate
//     map is one more static buffer of the same shape per attribute; mm_closed_kernel for a
//     closed rate-field pass, in which cells of rate zero are walls);
//   * a compute stream and a comm stream; with a halo (RCCL or host transport) each pass
//     runs the interior rows on the compute stream while the `depth` border rows wait
//     for the exchange on the comm stream (RCCL: ncclSend/ncclRecv of `depth` rows to
//     both neighbours; host: the caller imported them before mm_run);
//   * steps are captured once into a hipGraph (one ping-pong cycle, RCCL calls
//     included) and replayed; a refused capture is reported by mm_engine_info;
//   * per-step sums (MPI_Report) are reduced on the device into a growable history.
// This unit runs: streams, events, graph capture, RCCL and the launches. What a run does --
// kernel per pass, pass lengths, segments, launches, graph length, the MM_* knobs -- is
// planned in mm_plan.cpp (host-only) from the engine's mm::PlanIn; what the flow list means --
// its fused passes, the ring, the program's shape in that PlanIn -- is mm_program.cpp's
// (host-only too).
// The reference's per-worker body this replaces is src/Model.hpp:135-261.
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/mpimodel.h"
#include "mm_inst.hpp"
#include "mm_plan.hpp"
#include "mm_program.hpp"

static_assert(MM_FIELD_MAX_STEPS == mm::kFieldMaxSteps, "include/mpimodel.h: MM_FIELD_MAX_STEPS");
static_assert(MM_CLOSED_MAX_STEPS == mm::kClosedMaxSteps, "include/mpimodel.h: MM_CLOSED_MAX_STEPS");

namespace {

thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

#define MM_HIP(expr)                                                                      \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess)                                                             \
            return fail(MM_ERR_HIP, std::string(#expr ": ") + hipGetErrorString(e_));     \
    } while (0)

#define MM_NCCL(expr)                                                                     \
    do {                                                                                  \
        ncclResult_t r_ = (expr);                                                         \
        if (r_ != ncclSuccess)                                                            \
            return fail(MM_ERR_RCCL, std::string(#expr ": ") + ncclGetErrorString(r_));   \
    } while (0)

#define MM_TRY(expr)             \
    do {                         \
        int rc_ = (expr);        \
        if (rc_ != MM_OK) return rc_; \
    } while (0)

}  // namespace

struct mm_engine {
    mm_desc d{};
    int na = 1;
    long long pitch = 0;
    long long rows_alloc = 0;  // h + 2 * kGhost
    double* base = nullptr;
    size_t bytes = 0;
    double* buf[2][mm::kMaxAttr] = {};
    int cur = 0;
    // static rate fields (MM_FLOW_DIFFUSE_FIELD): one (h + 2*kGhost) x pitch buffer per
    // attribute that has one, allocated and zeroed on first use; fld points at owned row 0
    double* fld_base[mm::kMaxAttr] = {};
    double* fld[mm::kMaxAttr] = {};
    // ghost rows of each field written since its allocation, counted contiguously outward
    // from the slab: [a][0] rows -1, -2, ..., [a][1] rows h, h+1, ... A record for check_run's
    // refusal only -- it never feeds the plan (a plan depends on mm_desc, the creation
    // environment and the flow list alone)
    long long fld_rows[mm::kMaxAttr][2] = {};
    hipStream_t s_comp = nullptr, s_comm = nullptr;
    hipEvent_t ev_ready = nullptr, ev_halo = nullptr;
    hipEvent_t ev_comp_mark = nullptr, ev_comm_done = nullptr;
    bool comm_live = false;  // border work of this run is pending on the comm stream
    ncclComm_t comm = nullptr;

    std::vector<mm::Flow> flows;
    std::vector<mm::Pass> passes;  // mm::compile_passes(flows)

    mm::PlanIn pin;  // what the planner sees of the engine (mm_plan.hpp): slab, program shape,
                     // the MM_* knobs, the device; pin.split: interior / border split
    int th_env = 8;  // MM_ROWS_PER_WAVE as the environment asked; pin.knobs.th is the
                     // effective height, derived from it and the program (mm::set_program)
    std::map<const mm::KernelInst*, int> slots;  // occupancy cache (slots_per_cu)
    bool self_halo = false;  // test mode: one RCCL rank exchanges border rows with itself
    int variant = 0;  // kernel tuning variant (MM_KERNEL_VARIANT), 0 = default
    double* partials = nullptr;
    long long partials_cap = 0;
    double* hist = nullptr;
    unsigned long long* hist_n = nullptr;  // [0] history entries, [1] level-sum workgroups done
    long long hist_cap = 0;
    long long hist_host = 0;    // entries the enqueued work appends (host-side count)
    double* sum_tmp = nullptr;  // mm_sums scratch: nblocks partials + 1 result per attribute
    long long sum_blocks = 0;

    long long steps_done = 0;

    // graph cache: key = (parity, length, reduce_every, reduction phase); value = the
    // executable and whether one replay flips the ping-pong buffers
    std::map<std::tuple<int, long long, long long, long long>, std::pair<hipGraphExec_t, int>> graphs;

    // (a refused capture clears pin.knobs.graphs_ok: steps then run eagerly)
    int graph_state = 0;       // 0 none yet, 1 replaying, -1 capture refused
    long long graph_launches = 0;
    int graph_count = 0;
    std::string graph_note;

    bool timing = false;
    std::vector<hipEvent_t> ev_pool;
    std::vector<double> ev_bytes;  // algorithmic bytes of each timed launch (pairs of events)
    size_t ev_used = 0;
    long long timed_launches = 0;
    double timed_ms = 0.0;
    double timed_bytes = 0.0;
};

namespace {

int set_device(mm_engine* e) {
    MM_HIP(hipSetDevice(e->d.device));
    return MM_OK;
}

void drop_graphs(mm_engine* e) {
    for (auto& kv : e->graphs) (void)hipGraphExecDestroy(kv.second.first);
    e->graphs.clear();
}

void fill_args(const mm_engine* e, const mm::Pass& p, mm::PassArgs& A) {
    std::memset(&A, 0, sizeof A);
    for (int a = 0; a < e->na; ++a) {
        A.in[a] = e->buf[e->cur][a];
        A.out[a] = e->buf[e->cur ^ 1][a];
    }
    A.H = e->d.H;
    A.W = e->d.W;
    A.x_init = e->d.x_init;
    A.pitch = e->pitch;
    A.diffuse_mask = p.diffuse_mask;
    for (int a = 0; a < mm::kMaxAttr; ++a) A.drate[a] = p.drate[a];
    A.npre = (int)p.pre.size();
    A.npost = (int)p.post.size();
    for (size_t i = 0; i < p.pre.size(); ++i) {
        A.pre_a[i] = (signed char)p.pre[i].a;
        A.pre_b[i] = (signed char)p.pre[i].b;
        A.pre_r[i] = p.pre[i].rate;
    }
    for (size_t i = 0; i < p.post.size(); ++i) {
        A.post_a[i] = (signed char)p.post[i].a;
        A.post_b[i] = (signed char)p.post[i].b;
        A.post_r[i] = p.post[i].rate;
    }
    A.partials = e->partials;
    A.field_mask = p.field_mask;
    for (int a = 0; a < e->na; ++a) A.field[a] = ((p.field_mask >> a) & 1) ? e->fld[a] : nullptr;
}

hipEvent_t next_event(mm_engine* e) {
    if (e->ev_used == e->ev_pool.size()) {
        hipEvent_t ev;
        if (hipEventCreate(&ev) != hipSuccess) return nullptr;
        e->ev_pool.push_back(ev);
    }
    return e->ev_pool[e->ev_used++];
}

// The key of the instance that runs a k-step pass of the engine's program (mm_inst.hpp).
// nt: non-temporal stores -- bit 0 of the tuning variant and no other bit of it, so no user
// value of MM_KERNEL_VARIANT selects the ring instance. A four-attribute wide pass adds what
// its instance has at compile time: the ring, a post-chain, the diffusing attributes
// (relabel puts them first).
mm::InstKey inst_key(const mm_engine* e, mm::Kernel kernel, int k, int cols, bool seg, bool red,
                     bool nt) {
    mm::InstKey q{};
    q.family = kernel == mm::kWide      ? mm::kInstWide
               : kernel == mm::kFieldK  ? mm::kInstFieldK
               : kernel == mm::kClosedK ? mm::kInstClosedK
                                        : mm::kInstPassK;
    q.k = k, q.cols = cols, q.na = e->na;
    q.seg = seg, q.red = red, q.nt = nt;
    if (kernel == mm::kWide && e->na > 1 && e->passes.size() == 1) {
        const mm::Pass& p = e->passes[0];
        q.ring = e->pin.ring;
        q.post = !p.post.empty();
        q.nd = __builtin_popcount((unsigned)p.diffuse_mask);
    }
    return q;
}

// Identity attribute permutation, packed 2 bits per slot (launch_finalize_levels).
constexpr int kPermIdentity = 0 | 1 << 2 | 2 << 4 | 3 << 6;

// A four-attribute wide pass runs an instance with its diffusing attributes first: the
// pass's arguments are relabelled so that physical slot i holds logical attribute perm[i]
// -- the diffusing attributes in order, then the others -- its buffers, rates and chain
// operands with them. Returns the permutation packed like kPermIdentity, for the step
// sums (partials come out in physical order; the history is logical).
int relabel(const mm_engine* e, mm::PassArgs& A) {
    if (e->na == 1) return kPermIdentity;
    const mm::Pass& p = e->passes[0];
    int perm[mm::kMaxAttr], inv[mm::kMaxAttr], n = 0;
    for (int a = 0; a < e->na; ++a)
        if ((p.diffuse_mask >> a) & 1) perm[n++] = a;
    const int nd = n;
    for (int a = 0; a < e->na; ++a)
        if (!((p.diffuse_mask >> a) & 1)) perm[n++] = a;
    int code = 0;
    for (int i = 0; i < e->na; ++i) {
        inv[perm[i]] = i;
        code |= perm[i] << (2 * i);
        A.in[i] = e->buf[e->cur][perm[i]];
        A.out[i] = e->buf[e->cur ^ 1][perm[i]];
        A.drate[i] = p.drate[perm[i]];
    }
    A.diffuse_mask = (1 << nd) - 1;
    for (size_t t = 0; t < p.pre.size(); ++t) {
        A.pre_a[t] = (signed char)inv[p.pre[t].a];
        A.pre_b[t] = (signed char)(p.pre[t].b < 0 ? -1 : inv[p.pre[t].b]);
    }
    for (size_t t = 0; t < p.post.size(); ++t) {
        A.post_a[t] = (signed char)inv[p.post[t].a];
        A.post_b[t] = (signed char)(p.post[t].b < 0 ? -1 : inv[p.post[t].b]);
    }
    return code;
}

// Resident slots per CU of the instance that runs a k-step pass (mm::PlanIn::slots): waves
// of mm_passk_kernel, workgroups of mm_wide_kernel, from the instance's registers and LDS,
// cached by instance. An unknown instance counts one slot, as a failed query does. cols: the
// wide kernel's columns per lane where not its usual ones (mm_wide6_kernel: mm::kWide6Cols).
int slots_per_cu(mm_engine* e, mm::Kernel kernel, int k, bool red, int cols = 0) {
    const bool wide = kernel == mm::kWide;
    if (!cols) cols = wide ? (e->na > 1 ? 2 : 4) : 2;
    const mm::KernelInst* inst =
        mm::find_inst(inst_key(e, kernel, k, cols, true, red, e->variant & 1));
    if (!inst) return 1;
    int& s = e->slots[inst];
    if (!s) s = std::max(1, mm::inst_blocks_per_cu(*inst) * (wide ? 1 : mm::kWavesPerBlock));
    return s;
}

// The slab has a halo: a neighbour, or a halo mode on one slab (the self-halo among them).
bool field_halo(const mm_engine* e) { return e->d.nranks > 1 || e->d.halo_mode != MM_HALO_NONE; }

// After every change of the flow list: its passes, and the program's shape for the planner.
void set_program(mm_engine* e) {
    e->passes = mm::compile_passes(e->flows);
    mm::set_program(e->pin, e->passes, field_halo(e), e->th_env);
}

// Border-row exchange with both neighbours in one RCCL group: the first / last `depth`
// owned rows go to rank-1 / rank+1, their rows land in the ghost rows. Rows are
// contiguous (pitch doubles each), so every message is one contiguous block. The
// engine keeps depth <= min_rows, so the sent rows are always owned rows.
int halo_rccl(mm_engine* e, int depth) {
    const int r = e->d.rank, n = e->d.nranks;
    const long long P = e->pitch, h = e->d.h;
    const size_t cnt = (size_t)(depth * P);
    MM_NCCL(ncclGroupStart());
    for (int a = 0; a < e->na; ++a) {
        double* b = e->buf[e->cur][a];
        if (e->self_halo) {
            // one rank, both neighbours itself: the first rows land in the bottom ghost
            // rows and the last rows in the top ghost rows. Those ghost rows lie outside
            // the grid, so the kernels never read them as cells: the exchange exercises
            // the RCCL path without changing the result.
            MM_NCCL(ncclSend(b, cnt, ncclDouble, 0, e->comm, e->s_comm));
            MM_NCCL(ncclSend(b + (h - depth) * P, cnt, ncclDouble, 0, e->comm, e->s_comm));
            MM_NCCL(ncclRecv(b + h * P, cnt, ncclDouble, 0, e->comm, e->s_comm));
            MM_NCCL(ncclRecv(b - depth * P, cnt, ncclDouble, 0, e->comm, e->s_comm));
            continue;
        }
        if (r > 0) {
            MM_NCCL(ncclSend(b, cnt, ncclDouble, r - 1, e->comm, e->s_comm));
            MM_NCCL(ncclRecv(b - depth * P, cnt, ncclDouble, r - 1, e->comm, e->s_comm));
        }
        if (r < n - 1) {
            MM_NCCL(ncclSend(b + (h - depth) * P, cnt, ncclDouble, r + 1, e->comm, e->s_comm));
            MM_NCCL(ncclRecv(b + h * P, cnt, ncclDouble, r + 1, e->comm, e->s_comm));
        }
    }
    MM_NCCL(ncclGroupEnd());
    return MM_OK;
}

bool rccl_halo(const mm_engine* e) { return e->comm != nullptr; }

// Start of a split pass. Two streams per pass, joined by events:
//   comm:    [RCCL exchange k (right after border k-1)] -> [after interior k-1] border k
//   compute: [after border k-1] interior k
// so the exchange and the border rows run beside the interior kernels. Interior k reads
// rows border k-1 wrote; border k reads rows interior k-1 wrote and writes rows interior
// k-1 read; ghost rows are only touched on comm; the rows an exchange sends were written
// by the border kernel before it. With the host transport the caller has already put the
// neighbours' rows into the ghost rows, and the same schedule runs without the exchange.
// A split pass in two halves, the compute stream's first: the interior rows need only the
// previous border rows, not this pass's exchange, so their launch goes ahead of the
// exchange's host-side enqueue (an RCCL group call took 64 us before the interior's launch
// in profiles/r06/trace20).
int split_comp(mm_engine* e) {
    // interior k reads the rows border k-1 wrote
    if (e->comm_live) MM_HIP(hipStreamWaitEvent(e->s_comp, e->ev_comm_done, 0));
    // everything the compute stream ran before interior k: interior k-1, the fills
    MM_HIP(hipEventRecord(e->ev_comp_mark, e->s_comp));
    return MM_OK;
}

int split_comm(mm_engine* e, int depth) {
    // first split pass of the run: the exchange follows all earlier compute work
    if (!e->comm_live) MM_HIP(hipStreamWaitEvent(e->s_comm, e->ev_comp_mark, 0));
    if (rccl_halo(e)) MM_TRY(halo_rccl(e, depth));  // needs only border k-1 (same stream)
    // border k reads rows interior k-1 wrote (and reuses the partials finalize k-1 read)
    MM_HIP(hipStreamWaitEvent(e->s_comm, e->ev_comp_mark, 0));
    return MM_OK;
}

// Slab too thin to split: exchange first, then one launch on the compute stream.
int unsplit_halo(mm_engine* e, int depth) {
    if (!rccl_halo(e)) return MM_OK;
    MM_HIP(hipEventRecord(e->ev_ready, e->s_comp));
    MM_HIP(hipStreamWaitEvent(e->s_comm, e->ev_ready, 0));
    MM_TRY(halo_rccl(e, depth));
    MM_HIP(hipEventRecord(e->ev_halo, e->s_comm));
    MM_HIP(hipStreamWaitEvent(e->s_comp, e->ev_halo, 0));
    return MM_OK;
}

// One kernel launch of a pass on a stream. A border launch takes no tuning variant.
int launch(mm_engine* e, const mm::PassLaunches& pl, bool red, const mm::PassArgs& A, hipStream_t s,
           bool border, bool closed) {
    const int nt = border ? 0 : e->variant;
    if (pl.kern.kernel != mm::kOneStep)  // mm_passk_kernel, mm_wide_kernel, mm_fieldk_kernel,
                                         // mm_closedk_kernel
        MM_HIP(mm::launch_kstep(
            inst_key(e, pl.kern.kernel, pl.depth, pl.kern.cols, A.seg != 0, red, nt & 1), A, s));
    else if (closed)  // a closed rate-field pass
        MM_HIP(mm::launch_closed(e->na, red, A, s, nt));
    else if (A.field_mask)  // a rate-field pass
        MM_HIP(mm::launch_field(e->na, red, A, s, nt));
    else
        MM_HIP(mm::launch_pass(e->na, red, A, s, e->variant));
    return MM_OK;
}

void set_launch(mm::PassArgs& A, const mm::Launch& l) {
    A.ra0 = (int)l.lo, A.ra1 = (int)l.hi, A.rb0 = (int)l.lo2, A.rb1 = (int)l.hi2;
    A.seg = l.seg, A.th = l.th, A.th_edge = l.th_edge, A.xcd_remap = l.xcd_remap;
    A.nstrips = l.nstrips;
    A.waves_a = l.waves_a, A.waves_total = l.waves_total, A.partial_base = l.partial_base;
    const mm::Wide6& w = l.c6;  // the fused six-column pass (all 0 otherwise)
    A.c6_top = w.top, A.c6_bot = w.bot, A.c6_col = w.col, A.c6_rcol = w.rcol;
    A.c6_strips = w.strips, A.c6_rstrips = w.rstrips, A.c6_th = w.th;
    A.c6_band0 = w.band0, A.c6_band1 = w.band1, A.c6_frame = w.frame;
}

// One kernel pass over the slab, as mm::pass_launches describes it: k fused steps of the
// one-pass program p on mm_passk_kernel, mm_wide_kernel or mm_fieldk_kernel (bit j of `mask`: append the sums
// after step j+1 of the pass to the history), or pass p of one step on the one-step kernel
// (mask: append its sums). With a halo the interior rows run beside the exchange (every k
// steps, k rows deep), the border rows after it on the comm stream. time_it: an event pair
// around the interior launch (algorithmic bytes: every cell of its rows read once and
// written once per attribute). prime: mm_prepare's dispatches -- each launch of the pass
// once with no work (every workgroup leaves at its first instruction: waves_total = 0, the
// priming mark waves_a < 0), no exchange, no state change. A split pass also launches on
// the comm stream, another queue with its own scratch: unprimed, the first border launch of
// a 20-step run blocked the host for 1.5 ms (8192 x 32768 self-halo, profiles/r06/trace20).
int enqueue_pass(mm_engine* e, const mm::Pass& p, int k, int mask, bool time_it, bool prime = false) {
    const bool red = mask != 0;
    const mm::PassLaunches pl = mm::pass_launches(e->pin, k, red);
    mm::PassArgs A;
    fill_args(e, p, A);
    const int perm = pl.kern.kernel == mm::kWide ? relabel(e, A) : kPermIdentity;
    mm::PassArgs B = A;
    set_launch(A, pl.interior);
    set_launch(B, pl.border);
    if (prime) {
        A.waves_total = B.waves_total = 0;
        A.waves_a = B.waves_a = -1;
        MM_TRY(launch(e, pl, red, A, e->s_comp, false, p.closed));
        if (pl.split) MM_TRY(launch(e, pl, red, B, e->s_comm, true, p.closed));
        return MM_OK;
    }
    if (pl.split)
        MM_TRY(split_comp(e));
    else if (e->pin.split)
        MM_TRY(unsplit_halo(e, pl.depth));
    hipEvent_t t0 = nullptr, t1 = nullptr;
    if (time_it) {
        t0 = next_event(e);
        t1 = next_event(e);
        if (!t0 || !t1) return fail(MM_ERR_HIP, "hipEventCreate failed");
        e->ev_bytes.resize(e->ev_used / 2);
        // a rate-field attribute also reads its field: 24 B per cell
        e->ev_bytes.back() = (16.0 * e->na + 8.0 * __builtin_popcount((unsigned)p.field_mask)) *
                             (double)(pl.interior.hi - pl.interior.lo) * (double)e->d.W;
        MM_HIP(hipEventRecord(t0, e->s_comp));
    }
    MM_TRY(launch(e, pl, red, A, e->s_comp, false, p.closed));
    if (time_it) MM_HIP(hipEventRecord(t1, e->s_comp));
    if (pl.split) {
        MM_TRY(split_comm(e, pl.depth));
        MM_TRY(launch(e, pl, red, B, e->s_comm, true, p.closed));
        MM_HIP(hipEventRecord(e->ev_comm_done, e->s_comm));
        e->comm_live = true;
        if (red) MM_HIP(hipStreamWaitEvent(e->s_comp, e->ev_comm_done, 0));
    }
    if (red && pl.kern.kernel == mm::kOneStep)
        MM_HIP(mm::launch_finalize(e->partials, pl.total, e->na, e->hist, e->hist_n, e->hist_cap,
                                   e->s_comp, 1));
    else if (red)
        MM_HIP(mm::launch_finalize_levels(e->partials, pl.total, k, e->na, mask, e->hist,
                                          e->hist_n, e->hist_cap, e->s_comp, perm));
    e->cur ^= 1;
    return MM_OK;
}

// Enqueue steps [first, first+n) of a run (1-based step numbers decide the reductions).
int enqueue_steps(mm_engine* e, long long first, long long n, long long reduce_every,
                  bool time_it) {
    long long s = first;
    const long long end = first + n;
    auto red = [&](long long step) { return reduce_every > 0 && step % reduce_every == 0; };
    if (mm::kstep_ok(e->pin)) {
        for (int k : mm::pass_lengths(e->pin, n)) {
            int mask = 0;
            for (int j = 0; j < k; ++j)
                if (red(s + j)) mask |= 1 << j;
            MM_TRY(enqueue_pass(e, e->passes[0], k, mask, time_it));
            s += k;
        }
    } else {  // one step: all its passes; the last one appends the sums
        const int np = (int)e->passes.size();
        for (; s < end; ++s)
            for (int pi = 0; pi < np; ++pi)
                MM_TRY(enqueue_pass(e, e->passes[pi], 1, red(s) && pi == np - 1, time_it));
    }
    // the compute stream is the tail of every run (and of every captured graph)
    if (e->comm_live) {
        MM_HIP(hipStreamWaitEvent(e->s_comp, e->ev_comm_done, 0));
        e->comm_live = false;
    }
    return MM_OK;
}

// Every rank of an RCCL chain must run the same passes, or the K-row exchanges would not
// pair up: a graph replays the passes of its length, the eager fallback plans the rest of
// the run. So whether a capture worked is agreed over the chain (one all-reduce of a flag,
// at the first capture of each graph: every rank captures the same keys at the same call,
// which needs the same MM_GRAPH setting, timing mode and run lengths on every rank --
// include/mpimodel.h). The all-reduce shares the communicator with the halo send / recv
// of earlier runs, which may still be replaying on the compute stream: both streams are
// drained first, so no two RCCL operations of this communicator are in flight at once.
int agree_capture(mm_engine* e, bool ok) {
    if (!e->comm || e->d.nranks <= 1) return ok ? MM_OK : MM_ERR_HIP;
    int v = ok ? 1 : 0;
    int* dv = reinterpret_cast<int*>(e->sum_tmp);
    if (hipStreamSynchronize(e->s_comp) != hipSuccess ||
        hipStreamSynchronize(e->s_comm) != hipSuccess ||
        hipMemcpy(dv, &v, sizeof v, hipMemcpyHostToDevice) != hipSuccess ||
        ncclAllReduce(dv, dv, 1, ncclInt32, ncclMin, e->comm, e->s_comm) != ncclSuccess ||
        hipStreamSynchronize(e->s_comm) != hipSuccess ||
        hipMemcpy(&v, dv, sizeof v, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(MM_ERR_RCCL, "capture agreement all-reduce failed");
    if (v) return MM_OK;
    return ok ? fail(MM_ERR_HIP, "another rank's stream capture was refused") : MM_ERR_HIP;
}

int capture_graph(mm_engine* e, long long len, long long reduce_every, long long phase,
                  hipGraphExec_t* out, int* flip);

int get_graph(mm_engine* e, long long len, long long reduce_every, long long phase,
              hipGraphExec_t* out, int* flip) {
    auto key = std::make_tuple(e->cur, len, reduce_every, phase);
    auto it = e->graphs.find(key);
    if (it != e->graphs.end()) {
        *out = it->second.first;
        *flip = it->second.second;
        return MM_OK;
    }
    const int rc = capture_graph(e, len, reduce_every, phase, out, flip);
    const std::string why = g_last_error;
    const int ra = agree_capture(e, rc == MM_OK);
    if (rc != MM_OK) g_last_error = why;
    return rc != MM_OK ? rc : ra;
}

int capture_graph(mm_engine* e, long long len, long long reduce_every, long long phase,
                  hipGraphExec_t* out, int* flip) {
    auto key = std::make_tuple(e->cur, len, reduce_every, phase);
    const int cur0 = e->cur;
    MM_HIP(hipStreamBeginCapture(e->s_comp, hipStreamCaptureModeThreadLocal));
    const int rc = enqueue_steps(e, phase + 1, len, reduce_every, false);
    hipGraph_t g = nullptr;
    hipError_t ec = hipStreamEndCapture(e->s_comp, &g);
    const int parity = e->cur ^ cur0;  // the captured passes' buffer flips, mod 2
    e->cur = cur0;  // capture only recorded the work; the state advances at replay
    e->comm_live = false;
    if (rc != MM_OK) {
        if (g) (void)hipGraphDestroy(g);
        return rc;
    }
    if (ec != hipSuccess) return fail(MM_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ec));
    hipGraphExec_t ge = nullptr;
    ec = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (ec != hipSuccess) return fail(MM_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(ec));
    e->graphs[key] = std::make_pair(ge, parity);
    e->graph_count += 1;
    *out = ge;
    *flip = parity;
    return MM_OK;
}

int ensure_partials(mm_engine* e) {
    const long long need = mm::partials_need(e->pin);
    if (need <= e->partials_cap) return MM_OK;
    if (e->partials) (void)hipFree(e->partials);
    e->partials = nullptr;
    MM_HIP(hipMalloc(&e->partials, sizeof(double) * (size_t)need));
    e->partials_cap = need;
    return MM_OK;
}

// Make room for `more` history entries beyond the ones already enqueued. The history
// pointer is captured by the step graphs, so growing it drops them.
int reserve_history(mm_engine* e, long long more) {
    const long long need = e->hist_host + more;
    if (need <= e->hist_cap) return MM_OK;
    const long long cap = std::max(need, 2 * e->hist_cap);
    double* nh = nullptr;
    MM_HIP(hipStreamSynchronize(e->s_comp));
    MM_HIP(hipStreamSynchronize(e->s_comm));
    MM_HIP(hipMalloc(&nh, sizeof(double) * (size_t)cap * e->na));
    MM_HIP(hipMemcpyAsync(nh, e->hist, sizeof(double) * (size_t)e->hist_cap * e->na,
                          hipMemcpyDeviceToDevice, e->s_comp));
    MM_HIP(hipStreamSynchronize(e->s_comp));
    (void)hipFree(e->hist);
    e->hist = nh;
    e->hist_cap = cap;
    drop_graphs(e);
    return MM_OK;
}

int copy_rows(mm_engine* e, bool to_host, long long row0, int nrows, double* host) {
    const long long W = e->d.W, P = e->pitch;
    for (int a = 0; a < e->na; ++a) {
        double* dev = e->buf[e->cur][a] + row0 * P;
        double* hp = host + (size_t)a * nrows * W;
        if (to_host)
            MM_HIP(hipMemcpy2DAsync(hp, sizeof(double) * W, dev, sizeof(double) * P,
                                    sizeof(double) * W, nrows, hipMemcpyDeviceToHost, e->s_comp));
        else
            MM_HIP(hipMemcpy2DAsync(dev, sizeof(double) * P, hp, sizeof(double) * W,
                                    sizeof(double) * W, nrows, hipMemcpyHostToDevice, e->s_comp));
    }
    return MM_OK;
}

}  // namespace

extern "C" {

int mm_abi_version(void) { return MM_ABI_VERSION; }

const char* mm_last_error(void) { return g_last_error.c_str(); }

long long mm_step_count(double time, double time_step) {
    if (!(time_step > 0.0)) return -1;  // the reference would loop forever
    long long n = 0;
    for (double t = 0; t < time; t = t + time_step) ++n;  // src/Model.hpp:48, same fp64 sequence
    return n;
}

int mm_partition_reference(int H, int W, int P, int k, int* x_init, int* y_init, int* height,
                           int* width) {
    if (H <= 0 || W <= 0 || P <= 0 || k < 1 || k > P || !x_init || !y_init || !height || !width)
        return fail(MM_ERR_INVALID, "mm_partition_reference: bad arguments");
    const int count = (H * W) / P;  // src/Model.hpp:63
    const int offset = (k - 1) * count;
    *x_init = offset / W;  // src/Model.hpp:72
    *y_init = 0;
    *height = H / P;
    *width = W;
    return MM_OK;
}

int mm_owner_reference(int H, int P, int x) {
    if (H <= 0 || P <= 0 || H / P == 0) return -1;
    return x / (H / P) + 1;  // src/Model.hpp:80
}

int mm_partition_rows(long long H, int G, int g, long long* x_init, long long* h) {
    if (H <= 0 || G <= 0 || g < 0 || g >= G || !x_init || !h)
        return fail(MM_ERR_INVALID, "mm_partition_rows: bad arguments");
    const long long a = (g * H) / G, b = ((g + 1) * H) / G;
    *x_init = a;
    *h = b - a;
    return MM_OK;
}

int mm_neighbor_count(long long H, long long W, long long x, long long y) {
    const long long sx = mm::span3(H, x), sy = mm::span3(W, y);
    return (sx && sy) ? (int)(sx * sy - 1) : 0;
}

int mm_comm_id_size(void) { return (int)sizeof(ncclUniqueId); }

int mm_comm_id_create(void* out, int len) {
    if (!out || len < (int)sizeof(ncclUniqueId)) return fail(MM_ERR_INVALID, "mm_comm_id_create: buffer too small");
    ncclUniqueId id;
    MM_NCCL(ncclGetUniqueId(&id));
    std::memcpy(out, &id, sizeof id);
    return MM_OK;
}

int mm_device_synchronize(int device) {
    MM_HIP(hipSetDevice(device));
    MM_HIP(hipDeviceSynchronize());
    return MM_OK;
}

int mm_device_count(int* n) {
    if (!n) return fail(MM_ERR_INVALID, "mm_device_count: null");
    MM_HIP(hipGetDeviceCount(n));
    return MM_OK;
}

int mm_engine_create(const mm_desc* desc, mm_engine** out) {
    if (!desc || !out) return fail(MM_ERR_INVALID, "mm_engine_create: null argument");
    *out = nullptr;
    const mm_desc& d = *desc;
    if (d.H <= 0 || d.W <= 0 || d.h <= 0 || d.x_init < 0 || d.x_init + d.h > d.H)
        return fail(MM_ERR_INVALID, "mm_engine_create: slab outside the grid");
    if (d.n_attr < 1 || d.n_attr > mm::kMaxAttr)
        return fail(MM_ERR_INVALID, "mm_engine_create: n_attr must be 1..4");
    if (d.nranks < 1 || d.rank < 0 || d.rank >= d.nranks)
        return fail(MM_ERR_INVALID, "mm_engine_create: bad rank/nranks");
    if (d.nranks == 1 && (d.x_init != 0 || d.h != d.H))
        return fail(MM_ERR_INVALID, "mm_engine_create: a single slab must own the whole grid");
    if (d.halo_mode == MM_HALO_RCCL && !d.comm_id)
        return fail(MM_ERR_INVALID, "mm_engine_create: MM_HALO_RCCL needs comm_id");
    if (d.nranks > 1 && d.halo_mode == MM_HALO_NONE)
        return fail(MM_ERR_INVALID, "mm_engine_create: nranks > 1 needs a halo mode");
    if (d.W > (1LL << 30) || d.h > (1LL << 30))
        return fail(MM_ERR_INVALID, "mm_engine_create: slab too large");

    mm_engine* e = new mm_engine();
    e->d = d;
    e->na = d.n_attr;
    e->pitch = (d.W + mm::kStripCols - 1) / mm::kStripCols * mm::kStripCols;
    e->rows_alloc = d.h + 2 * mm::kGhost;
    mm::PlanIn& pin = e->pin;
    pin.H = d.H, pin.W = d.W, pin.h = d.h, pin.x_init = d.x_init, pin.nranks = d.nranks;
    pin.pitch = e->pitch, pin.n_attr = d.n_attr;
    // thinnest slab of the chain: mm_partition_rows slabs are at least floor(H/G) rows
    // (RCCL engines replace this with the chain's true minimum below)
    pin.min_rows = std::min<long long>(d.h, d.H / d.nranks);
    pin.knobs = mm::read_knobs([](const char* name) -> const char* { return std::getenv(name); });
    e->th_env = pin.knobs.th;
    pin.slots = [e](mm::Kernel kernel, int k, bool red) { return slots_per_cu(e, kernel, k, red); };
    pin.slots6 = [e](int k) { return slots_per_cu(e, mm::kWide, k, false, mm::kWide6Cols); };
    e->variant = mm::kernel_variant(pin);

    auto cleanup = [&](int rc) {
        mm_engine_destroy(e);
        return rc;
    };
    hipError_t he = hipSetDevice(d.device);
    if (he != hipSuccess) return cleanup(fail(MM_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(he)));
    he = hipDeviceGetAttribute(&e->pin.ncu, hipDeviceAttributeMultiprocessorCount, d.device);
    if (he != hipSuccess || e->pin.ncu <= 0) e->pin.ncu = 256;

    const size_t per = (size_t)e->rows_alloc * (size_t)e->pitch;  // doubles per buffer
    const size_t per_al = (per + 31) / 32 * 32;                   // 256-B aligned buffers
    e->bytes = sizeof(double) * per_al * 2 * (size_t)e->na;
    if (hipStreamCreateWithFlags(&e->s_comp, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&e->s_comm, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&e->ev_ready, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&e->ev_halo, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&e->ev_comp_mark, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&e->ev_comm_done, hipEventDisableTiming) != hipSuccess)
        return cleanup(fail(MM_ERR_HIP, "stream/event creation failed"));

    he = hipMalloc(&e->base, e->bytes);
    if (he != hipSuccess) return cleanup(fail(MM_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(he)));
    // zeroed on the compute stream: every fill, upload and pass is enqueued there (or, on
    // the comm stream, behind an event recorded there), so they all follow it. A zeroing
    // on the null stream would not be ordered before them -- the engine's streams are
    // non-blocking -- and once did land after a fill on memory another engine had just
    // freed (tests/test_gpu_parity.py::test_fill_after_freed_engine)
    he = hipMemsetAsync(e->base, 0, e->bytes, e->s_comp);
    if (he != hipSuccess) return cleanup(fail(MM_ERR_HIP, std::string("hipMemsetAsync: ") + hipGetErrorString(he)));
    for (int k = 0; k < 2; ++k)
        for (int a = 0; a < e->na; ++a)
            e->buf[k][a] = e->base + per_al * (size_t)(k * e->na + a) + mm::kGhost * e->pitch;

    int rc = ensure_partials(e);
    if (rc != MM_OK) return cleanup(rc);
    e->hist_cap = 1 << 12;
    if (hipMalloc(&e->hist, sizeof(double) * (size_t)e->hist_cap * e->na) != hipSuccess ||
        hipMalloc(&e->hist_n, 2 * sizeof(unsigned long long)) != hipSuccess ||
        hipMemsetAsync(e->hist_n, 0, 2 * sizeof(unsigned long long), e->s_comp) != hipSuccess)
        return cleanup(fail(MM_ERR_NOMEM, "history allocation failed"));
    e->sum_blocks = std::min<long long>(1024, std::max<long long>(1, d.h));
    if (hipMalloc(&e->sum_tmp, sizeof(double) * (size_t)(e->sum_blocks + mm::kMaxAttr)) != hipSuccess)
        return cleanup(fail(MM_ERR_NOMEM, "sum scratch allocation failed"));
    // the zeroing above is queued on the compute stream; waiting for it here keeps a
    // failure on this call (and costs no other engine anything: only this stream)
    he = hipStreamSynchronize(e->s_comp);
    if (he != hipSuccess) return cleanup(fail(MM_ERR_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(he)));

    e->self_halo = e->pin.knobs.self_halo && d.nranks == 1 && d.halo_mode == MM_HALO_RCCL;
    if ((d.nranks > 1 || e->self_halo) && d.halo_mode == MM_HALO_RCCL) {
        // a process that loaded another librccl.so.1 first (PyTorch bundles one) would
        // run this code against a different RCCL: refuse instead of crashing later
        int v = 0;
        if (ncclGetVersion(&v) != ncclSuccess || v != NCCL_VERSION_CODE) {
            char msg[160];
            std::snprintf(msg, sizeof msg,
                          "RCCL %d loaded, engine built against %d: load libmpimodel_hip.so "
                          "before any library that bundles its own librccl (e.g. torch)",
                          v, NCCL_VERSION_CODE);
            return cleanup(fail(MM_ERR_RCCL, msg));
        }
        ncclUniqueId id;
        std::memcpy(&id, d.comm_id, sizeof id);
        ncclResult_t nr = ncclCommInitRank(&e->comm, d.nranks, id, d.rank);
        if (nr != ncclSuccess)
            return cleanup(fail(MM_ERR_RCCL, std::string("ncclCommInitRank: ") + ncclGetErrorString(nr)));
        // the chain's thinnest slab (one setup-time collective): a depth-K exchange must
        // never send more rows than any rank owns
        long long hmin = d.h;
        double* dv = e->sum_tmp;
        if (hipMemcpy(dv, &hmin, sizeof hmin, hipMemcpyHostToDevice) != hipSuccess ||
            ncclAllReduce(dv, dv, 1, ncclInt64, ncclMin, e->comm, e->s_comm) != ncclSuccess ||
            hipStreamSynchronize(e->s_comm) != hipSuccess ||
            hipMemcpy(&hmin, dv, sizeof hmin, hipMemcpyDeviceToHost) != hipSuccess)
            return cleanup(fail(MM_ERR_RCCL, "min slab rows all-reduce failed"));
        e->pin.min_rows = hmin;
        e->pin.split = true;
    } else if (d.nranks > 1 && d.halo_mode == MM_HALO_HOST) {
        // the host transport sizes K and the halo depth from the standard partition
        // (min_rows above), so a neighbour of a caller-chosen thinner slab could be asked
        // for rows it does not own: only mm_partition_rows slabs are accepted
        long long x0 = 0, hh = 0;
        if (mm_partition_rows(d.H, d.nranks, d.rank, &x0, &hh) != MM_OK || x0 != d.x_init ||
            hh != d.h)
            return cleanup(fail(MM_ERR_INVALID, "mm_engine_create: MM_HALO_HOST slabs must be "
                                                "mm_partition_rows(H, nranks, rank)"));
        e->pin.split = true;
    }
    // default program: one Exponencial flow on attribute 0 is set by the caller
    *out = e;
    return MM_OK;
}

int mm_engine_destroy(mm_engine* e) {
    if (!e) return MM_OK;
    (void)hipSetDevice(e->d.device);
    if (e->s_comp) (void)hipStreamSynchronize(e->s_comp);
    if (e->s_comm) (void)hipStreamSynchronize(e->s_comm);
    drop_graphs(e);
    if (e->comm) (void)ncclCommDestroy(e->comm);
    for (hipEvent_t ev : e->ev_pool) (void)hipEventDestroy(ev);
    if (e->ev_ready) (void)hipEventDestroy(e->ev_ready);
    if (e->ev_halo) (void)hipEventDestroy(e->ev_halo);
    if (e->ev_comp_mark) (void)hipEventDestroy(e->ev_comp_mark);
    if (e->ev_comm_done) (void)hipEventDestroy(e->ev_comm_done);
    if (e->s_comp) (void)hipStreamDestroy(e->s_comp);
    if (e->s_comm) (void)hipStreamDestroy(e->s_comm);
    if (e->base) (void)hipFree(e->base);
    for (double* f : e->fld_base)
        if (f) (void)hipFree(f);
    if (e->partials) (void)hipFree(e->partials);
    if (e->hist) (void)hipFree(e->hist);
    if (e->hist_n) (void)hipFree(e->hist_n);
    if (e->sum_tmp) (void)hipFree(e->sum_tmp);
    (void)hipGetLastError();  // statuses above are ignored on purpose; do not leave them pending
    delete e;
    return MM_OK;
}

int mm_engine_info(mm_engine* e, mm_info* info) {
    if (!e || !info) return fail(MM_ERR_INVALID, "mm_engine_info: null");
    std::memset(info, 0, sizeof *info);
    info->pitch = e->pitch;
    info->bytes_device = (long long)e->bytes;
    info->n_passes = (int)e->passes.size();
    const mm::SlabPlan sp = mm::slab_plan(e->pin);
    info->kernel = sp.kernel;
    info->rows_per_wave = sp.rows_per_wave;
    info->waves_per_pass = sp.waves_per_pass;
    info->seg_waves_per_cu = sp.seg_waves_per_cu;
    if (sp.kernel == mm::kWide && e->na > 1)
        info->chain_kernel = (e->pin.ring && sp.steps_per_launch == 8) ? MM_CHAIN_RING : MM_CHAIN_RUNTIME;
    info->steps_done = e->steps_done;
    info->fused_attrs = e->na;
    info->steps_per_launch = info->halo_depth = sp.steps_per_launch;
    info->graph_state = e->graph_state;
    info->graph_count = e->graph_count;
    info->graph_launches = e->graph_launches;
    info->hist_entries = e->hist_host;
    std::snprintf(info->graph_note, sizeof info->graph_note, "%s", e->graph_note.c_str());
    return MM_OK;
}

int mm_fill(mm_engine* e, int attr, int mode, double value, unsigned long long seed) {
    if (!e || attr < 0 || attr >= e->na || (mode != MM_FILL_UNIFORM && mode != MM_FILL_RANDOM))
        return fail(MM_ERR_INVALID, "mm_fill: bad arguments");
    MM_TRY(set_device(e));
    MM_HIP(mm::launch_fill(e->buf[e->cur][attr], e->pitch, e->d.H, e->d.W, e->d.x_init, e->d.h,
                           mode, value, seed, e->s_comp));
    MM_HIP(hipStreamSynchronize(e->s_comp));
    e->steps_done = 0;
    return MM_OK;
}

int mm_upload(mm_engine* e, int attr, const double* host) {
    if (!e || !host || attr < 0 || attr >= e->na) return fail(MM_ERR_INVALID, "mm_upload: bad arguments");
    MM_TRY(set_device(e));
    MM_HIP(hipMemcpy2DAsync(e->buf[e->cur][attr], sizeof(double) * e->pitch, host,
                            sizeof(double) * e->d.W, sizeof(double) * e->d.W, e->d.h,
                            hipMemcpyHostToDevice, e->s_comp));
    MM_HIP(hipStreamSynchronize(e->s_comp));
    e->steps_done = 0;
    return MM_OK;
}

int mm_download(mm_engine* e, int attr, double* host) {
    if (!e || !host || attr < 0 || attr >= e->na) return fail(MM_ERR_INVALID, "mm_download: bad arguments");
    MM_TRY(set_device(e));
    MM_HIP(hipStreamSynchronize(e->s_comm));
    MM_HIP(hipMemcpy2DAsync(host, sizeof(double) * e->d.W, e->buf[e->cur][attr],
                            sizeof(double) * e->pitch, sizeof(double) * e->d.W, e->d.h,
                            hipMemcpyDeviceToHost, e->s_comp));
    MM_HIP(hipStreamSynchronize(e->s_comp));
    return MM_OK;
}

int mm_clear_flows(mm_engine* e) {
    if (!e) return fail(MM_ERR_INVALID, "mm_clear_flows: null");
    MM_TRY(set_device(e));
    MM_HIP(hipStreamSynchronize(e->s_comp));
    e->flows.clear();
    set_program(e);
    drop_graphs(e);
    return MM_OK;
}

int mm_add_flow(mm_engine* e, int kind, int a, int b, double rate) {
    if (!e) return fail(MM_ERR_INVALID, "mm_add_flow: null");
    if (kind != MM_FLOW_DIFFUSE && kind != MM_FLOW_TRANSFER && kind != MM_FLOW_DIFFUSE_FIELD &&
        kind != MM_FLOW_DIFFUSE_CLOSED)
        return fail(MM_ERR_INVALID, "mm_add_flow: unknown flow kind");
    if (a < 0 || a >= e->na) return fail(MM_ERR_INVALID, "mm_add_flow: attribute out of range");
    if (kind == MM_FLOW_TRANSFER && b >= e->na)
        return fail(MM_ERR_INVALID, "mm_add_flow: target attribute out of range");
    // the rate is the attribute's field
    if (kind == MM_FLOW_DIFFUSE_FIELD || kind == MM_FLOW_DIFFUSE_CLOSED) rate = 0.0;
    if (!std::isfinite(rate)) return fail(MM_ERR_INVALID, "mm_add_flow: rate must be finite");
    MM_TRY(set_device(e));
    MM_HIP(hipStreamSynchronize(e->s_comp));
    e->flows.push_back({kind, a, kind == MM_FLOW_TRANSFER ? (b < 0 ? -1 : b) : a, rate});
    drop_graphs(e);
    set_program(e);
    return MM_OK;
}

}  // extern "C"

namespace {

// The rate field of one attribute, allocated and zeroed on first use. The step graphs
// capture the field pointers, so a new field drops them.
int ensure_field(mm_engine* e, int attr) {
    if (e->fld[attr]) return MM_OK;
    const size_t n = sizeof(double) * (size_t)e->rows_alloc * (size_t)e->pitch;
    double* p = nullptr;
    if (hipMalloc(&p, n) != hipSuccess) {
        (void)hipGetLastError();
        return fail(MM_ERR_NOMEM, "rate field allocation failed");
    }
    e->fld_base[attr] = p;
    e->fld[attr] = p + mm::kGhost * e->pitch;
    e->bytes += n;
    MM_HIP(hipMemsetAsync(p, 0, n, e->s_comp));
    MM_HIP(hipStreamSynchronize(e->s_comp));
    drop_graphs(e);
    return MM_OK;
}

}  // namespace

extern "C" {

int mm_rate_field_upload(mm_engine* e, int attr, long long row0, long long nrows,
                         const double* host) {
    if (!e || !host || attr < 0 || attr >= e->na || nrows < 0 || row0 < -mm::kGhost ||
        row0 + nrows > e->d.h + mm::kGhost)
        return fail(MM_ERR_INVALID, "mm_rate_field_upload: bad attribute, or rows outside the "
                                    "slab + ghost rows");
    const long long W = e->d.W;
    for (long long i = 0; i < nrows * W; ++i)
        if (!std::isfinite(host[i]))
            return fail(MM_ERR_INVALID, "mm_rate_field_upload: rates must be finite");
    MM_TRY(set_device(e));
    MM_TRY(ensure_field(e, attr));
    // rows outside the global grid are skipped
    const long long lo = std::max(row0, -e->d.x_init);
    const long long hi = std::min(row0 + nrows, e->d.H - e->d.x_init);
    if (hi > lo) {
        // the running steps read the field: on the compute stream (every run ends there), or
        // on the comm stream behind an event the compute stream waits for
        MM_HIP(hipMemcpy2DAsync(e->fld[attr] + lo * e->pitch, sizeof(double) * e->pitch,
                                host + (lo - row0) * W, sizeof(double) * W, sizeof(double) * W,
                                (size_t)(hi - lo), hipMemcpyHostToDevice, e->s_comp));
        MM_HIP(hipStreamSynchronize(e->s_comp));
    }
    // the ghost rows this call wrote (or skipped as outside the grid), where they continue
    // the rows already there: rows [row0, end) reach past row -1 - top / h + bottom
    long long& top = e->fld_rows[attr][0];
    long long& bottom = e->fld_rows[attr][1];
    const long long end = row0 + nrows;
    if (row0 < -top && end >= -top) top = -row0;
    if (end > e->d.h + bottom && row0 <= e->d.h + bottom) bottom = end - e->d.h;
    return MM_OK;
}

int mm_rate_field_fill(mm_engine* e, int attr, double value) {
    if (!e || attr < 0 || attr >= e->na || !std::isfinite(value))
        return fail(MM_ERR_INVALID, "mm_rate_field_fill: bad attribute or non-finite rate");
    MM_TRY(set_device(e));
    MM_TRY(ensure_field(e, attr));
    MM_HIP(mm::launch_fill(e->fld[attr], e->pitch, e->d.H, e->d.W, e->d.x_init, e->d.h,
                           MM_FILL_UNIFORM, value, 0, e->s_comp));
    MM_HIP(hipStreamSynchronize(e->s_comp));
    e->fld_rows[attr][0] = e->fld_rows[attr][1] = mm::kGhost;  // every ghost row inside the grid
    return MM_OK;
}

int mm_point_apply(mm_engine* e, int attr, long long sx, long long sy, double captured,
                   double rate) {
    if (!e || attr < 0 || attr >= e->na) return fail(MM_ERR_INVALID, "mm_point_apply: bad arguments");
    if (sx < 0 || sy < 0 || sx >= e->d.H || sy >= e->d.W)
        return fail(MM_ERR_INVALID, "mm_point_apply: source cell outside the grid");
    MM_TRY(set_device(e));
    MM_HIP(mm::launch_point(e->buf[e->cur][attr], e->pitch, e->d.H, e->d.W, e->d.x_init, e->d.h,
                            sx, sy, captured, rate, e->s_comp));
    return MM_OK;
}

int mm_point_apply_strict(mm_engine* e, int attr, long long sx, long long sy, double captured,
                          double rate, int P, int* applied) {
    if (applied) *applied = 0;
    if (!e || e->d.H > INT32_MAX || e->d.W > INT32_MAX)
        return fail(MM_ERR_INVALID, "mm_point_apply_strict: bad arguments");
    const int ok = mm_point_strict_applies((int)e->d.H, (int)e->d.W, P, (int)sx, (int)sy);
    if (ok < 0) return fail(MM_ERR_INVALID, "mm_point_apply_strict: bad source or worker count");
    if (ok == 0) return MM_OK;  // the reference changes no cell here
    if (applied) *applied = 1;
    return mm_point_apply(e, attr, sx, sy, captured, rate);
}

}  // extern "C"

namespace {

// The field of attribute a holds the `depth` ghost rows that `reader` (the message's subject)
// reads on every side with a real neighbour, clipped to the grid; knob: how the caller
// promised them.
int check_field_rows(mm_engine* e, const char* who, int a, long long depth, const char* reader,
                     const char* knob) {
    const long long want[2] = {e->d.rank > 0 ? std::min<long long>(depth, e->d.x_init) : 0,
                               e->d.rank < e->d.nranks - 1
                                   ? std::min<long long>(depth, e->d.H - e->d.x_init - e->d.h)
                                   : 0};
    for (int side = 0; side < 2; ++side)
        if (e->fld_rows[a][side] < want[side]) {
            char msg[256];
            std::snprintf(msg, sizeof msg,
                          "%s: %s %lld ghost rows of the field of attribute %d %s the slab (%s), "
                          "%lld have been uploaded (mm_rate_field_upload / mm_rate_field_fill)",
                          who, reader, want[side], a, side == 0 ? "above" : "below", knob,
                          e->fld_rows[a][side]);
            return fail(MM_ERR_STATE, msg);
        }
    return MM_OK;
}

int check_run(mm_engine* e, long long nsteps, long long reduce_every, const char* who) {
    if (!e || nsteps < 0 || reduce_every < 0) return fail(MM_ERR_INVALID, std::string(who) + ": bad arguments");
    if (nsteps == 0) return MM_OK;
    if (e->passes.empty()) return fail(MM_ERR_STATE, std::string(who) + ": no flow added (mm_add_flow)");
    for (const mm::Pass& p : e->passes)
        for (int a = 0; a < e->na; ++a)
            if (((p.field_mask >> a) & 1) && !e->fld[a])
                return fail(MM_ERR_STATE, std::string(who) + ": a rate-field diffusion's attribute has "
                                          "no field (mm_rate_field_upload / mm_rate_field_fill)");
    // K-step rate-field passes with a halo read `depth` ghost rows of the field on every
    // side that has a real neighbour (a self-halo side has none: its ghost rows lie outside
    // the grid). The engine never exchanges the field: the caller promised the rows at
    // creation (MM_FIELD_HALO), and a run without them is refused before it leaves a trace.
    if (e->pin.field_k >= 2 && field_halo(e))
        MM_TRY(check_field_rows(e, who, 0, mm::steps_per_launch(e->pin),
                                "K-step rate-field passes read", "MM_FIELD_HALO"));
    // A closed pass counts open neighbours: the share of the neighbour's border row needs
    // that row's count, which reads the field one row further out. On a slab with a halo the
    // caller promises two ghost rows of the field at creation (MM_FIELD_HALO=2) and uploads
    // them on every side with a real neighbour; the plan itself never depends on either.
    // K-step closed passes read one row more than their depth: K + 1 (MM_CLOSED_HALO).
    if (e->pin.closed_k >= 2 && field_halo(e))
        MM_TRY(check_field_rows(e, who, 0, mm::steps_per_launch(e->pin) + 1,
                                "K-step closed passes read", "MM_CLOSED_HALO"));
    for (const mm::Pass& p : e->passes) {
        if (!p.closed || !field_halo(e)) continue;
        if (mm::closed_field_promise(e->pin.knobs) < 2)
            return fail(MM_ERR_STATE, std::string(who) + ": a closed diffusion on a slab with a halo "
                                      "reads two ghost rows of the field: create the engine with "
                                      "MM_FIELD_HALO=2 (or more) and upload rows -2..h+1");
        MM_TRY(check_field_rows(e, who, __builtin_ctz((unsigned)p.field_mask), 2,
                                "a closed diffusion reads", "MM_FIELD_HALO=2"));
    }
    if (e->d.halo_mode == MM_HALO_HOST && e->d.nranks > 1) {
        if (e->passes.size() != 1)
            return fail(MM_ERR_STATE, std::string(who) + ": the host halo transport runs one-pass flow programs only");
        // one pass per call: the pass planner's length for nsteps (<= kGhost rows exchanged)
        if (nsteps > mm::kGhost || mm::next_pass_len(e->pin, nsteps) != nsteps)
            return fail(MM_ERR_STATE, std::string(who) + ": host halo transport: one pass per call "
                                      "(mm_pass_plan's pass lengths; exchange that many rows between calls)");
    }
    return MM_OK;
}

}  // namespace

extern "C" {

int mm_prepare(mm_engine* e, long long nsteps, long long reduce_every) {
    MM_TRY(check_run(e, nsteps, reduce_every, "mm_prepare"));
    if (nsteps == 0) return MM_OK;
    MM_TRY(set_device(e));
    const long long phase = reduce_every > 0 ? e->steps_done % reduce_every : 0;
    // the history the run appends, grown now: growing it inside mm_run would drop (and
    // re-capture) the graph prepared here
    const long long entries =
        reduce_every > 0 ? (phase + nsteps) / reduce_every - phase / reduce_every : 0;
    MM_TRY(reserve_history(e, entries));
    const long long per = e->timing ? 0 : mm::graph_per(e->pin, nsteps, reduce_every);
    long long tail = nsteps;
    if (per > 0) {
        // both buffer parities: untimed warmup steps run after mm_prepare may leave the
        // state at either one (graphs are keyed by the parity they start from)
        const int cur0 = e->cur;
        for (int par = 0; par < 2 && e->pin.knobs.graphs_ok; ++par) {
            e->cur = cur0 ^ par;
            hipGraphExec_t g = nullptr;
            int flip = 0;
            if (get_graph(e, per, reduce_every, phase, &g, &flip) != MM_OK) {
                e->graph_note = g_last_error;
                (void)hipGetLastError();
                e->pin.knobs.graphs_ok = false;
                e->graph_state = -1;
            } else {
                MM_HIP(hipGraphUpload(g, e->s_comp));  // the first launch then uploads nothing
                tail = nsteps % per;
            }
        }
        e->cur = cur0;
        MM_HIP(hipStreamSynchronize(e->s_comp));
    }
    // the eagerly launched passes: plan them now, which loads their kernels' code objects,
    // and dispatch each planned kernel once with no work (enqueue_pass's priming mode), so
    // the queue's scratch is sized for it here and not by the first timed pass (the K = 20
    // kernel keeps a few hundred bytes of scratch per lane in its GEN code: its first
    // dispatch started 172 us after its launch, profiles/r06/hiptrace). No step runs: no
    // buffer is read or written.
    if (mm::kstep_ok(e->pin) && tail > 0) {
        // the instances primed: each pass's own, with the step sums where one of its steps
        // is reduced and without where none is (a run may use both), the interior's on the
        // compute stream and a split pass's border instance on the comm stream
        long long s = phase + (nsteps - tail) + 1;
        for (int k : mm::pass_lengths(e->pin, tail)) {
            int red = 0;
            for (int j = 0; j < k; ++j) red |= reduce_every > 0 && (s + j) % reduce_every == 0;
            MM_TRY(enqueue_pass(e, e->passes[0], k, red, false, true));
            s += k;
        }
        MM_HIP(hipStreamSynchronize(e->s_comp));
        if (e->pin.split) MM_HIP(hipStreamSynchronize(e->s_comm));
    }
    return MM_OK;
}

int mm_pass_plan(mm_engine* e, long long nsteps, int* lens, int cap, int* count) {
    if (!e || nsteps < 0 || cap < 0 || (cap > 0 && !lens) || !count)
        return fail(MM_ERR_INVALID, "mm_pass_plan: bad arguments");
    if (e->passes.empty()) return fail(MM_ERR_STATE, "mm_pass_plan: no flow added (mm_add_flow)");
    const std::vector<int> plan = mm::pass_lengths(e->pin, nsteps);
    std::copy_n(plan.begin(), std::min<size_t>(plan.size(), (size_t)cap), lens);
    *count = (int)plan.size();
    return MM_OK;
}

int mm_pass_kernel(mm_engine* e, int k, int* kernel, int* cols_per_lane, long long* strips) {
    if (!e || k < 1 || !kernel || !cols_per_lane || !strips)
        return fail(MM_ERR_INVALID, "mm_pass_kernel: bad arguments");
    if (e->passes.empty()) return fail(MM_ERR_STATE, "mm_pass_kernel: no flow added (mm_add_flow)");
    const mm::KernelChoice kc = mm::kernel_for(e->pin, k);
    *kernel = kc.kernel;
    *cols_per_lane = kc.cols;
    *strips = kc.strips;
    return MM_OK;
}

int mm_run(mm_engine* e, long long nsteps, long long reduce_every) {
    MM_TRY(check_run(e, nsteps, reduce_every, "mm_run"));
    if (nsteps == 0) return MM_OK;
    MM_TRY(set_device(e));
    // steps are numbered from the last fill / upload on, so a run split into several
    // calls reduces the same steps as one call
    const long long phase = reduce_every > 0 ? e->steps_done % reduce_every : 0;
    const long long entries =
        reduce_every > 0 ? (phase + nsteps) / reduce_every - phase / reduce_every : 0;
    MM_TRY(reserve_history(e, entries));
    auto finish = [&]() {
        e->steps_done += nsteps;
        e->hist_host += entries;
        return MM_OK;
    };
    // eager launches plan their passes in the graph path's blocks (graph_per ignoring
    // graphs_ok / timing), so a rank whose capture was refused, or that times its
    // kernels, runs the same pass sequence -- the same K-row exchanges -- as the others
    auto eager = [&](bool timed) -> int {
        const long long pp = mm::graph_per(e->pin, nsteps, reduce_every, true);
        long long d = 0;
        if (pp > 0)
            for (; d + pp <= nsteps; d += pp) MM_TRY(enqueue_steps(e, phase + d + 1, pp, reduce_every, timed));
        if (d < nsteps) MM_TRY(enqueue_steps(e, phase + d + 1, nsteps - d, reduce_every, timed));
        return MM_OK;
    };
    if (e->timing) {  // eager launches with an event pair around each step kernel
        MM_TRY(eager(true));
        return finish();
    }
    const long long per = mm::graph_per(e->pin, nsteps, reduce_every);
    if (per == 0) {
        MM_TRY(eager(false));
        return finish();
    }
    hipGraphExec_t g = nullptr;
    int flip = 0;
    if (get_graph(e, per, reduce_every, phase, &g, &flip) != MM_OK) {
        // stream capture refused (e.g. by the RCCL build): run the same steps eagerly and
        // say so in mm_engine_info (graph_state -1, graph_note)
        e->graph_note = g_last_error;
        (void)hipGetLastError();
        e->pin.knobs.graphs_ok = false;
        e->graph_state = -1;
        MM_TRY(eager(false));
        return finish();
    }
    e->graph_state = 1;
    long long done = 0;
    for (; done + per <= nsteps; done += per) {
        if (done > 0 && flip) {  // an odd graph replays at the other parity: its own graph
            MM_TRY(get_graph(e, per, reduce_every, phase, &g, &flip));
        }
        MM_HIP(hipGraphLaunch(g, e->s_comp));
        e->graph_launches += 1;
        e->cur ^= flip;
    }
    if (done < nsteps)
        MM_TRY(enqueue_steps(e, phase + done + 1, nsteps - done, reduce_every, false));
    return finish();
}

int mm_synchronize(mm_engine* e) {
    if (!e) return fail(MM_ERR_INVALID, "mm_synchronize: null");
    MM_TRY(set_device(e));
    if (e->pin.knobs.sync_spin) {
        // poll the completion signals: the blocking wait returns tens to hundreds of us after
        // the last kernel ends (a sleeping host thread), time the GPU then sits idle in a
        // timed region or before the next launch
        for (hipStream_t s : {e->s_comp, e->s_comm}) {
            hipError_t q;
            while ((q = hipStreamQuery(s)) == hipErrorNotReady) __builtin_ia32_pause();
            if (q != hipSuccess) MM_HIP(q);
        }
    }
    MM_HIP(hipStreamSynchronize(e->s_comp));
    MM_HIP(hipStreamSynchronize(e->s_comm));
    return MM_OK;
}

int mm_sums(mm_engine* e, double* out) {
    if (!e || !out) return fail(MM_ERR_INVALID, "mm_sums: null");
    MM_TRY(set_device(e));
    for (int a = 0; a < e->na; ++a)
        MM_HIP(mm::launch_slab_sum(e->buf[e->cur][a], e->pitch, e->d.W, e->d.h, e->sum_tmp,
                                   e->sum_blocks, e->sum_tmp + e->sum_blocks + a, e->s_comp));
    MM_HIP(hipMemcpyAsync(out, e->sum_tmp + e->sum_blocks, sizeof(double) * e->na,
                          hipMemcpyDeviceToHost, e->s_comp));
    MM_HIP(hipStreamSynchronize(e->s_comp));
    return MM_OK;
}

int mm_sums_history(mm_engine* e, double* out, long long max_entries, long long* n) {
    if (!e || !n || (max_entries > 0 && !out)) return fail(MM_ERR_INVALID, "mm_sums_history: bad arguments");
    MM_TRY(set_device(e));
    unsigned long long cnt = 0;
    MM_HIP(hipStreamSynchronize(e->s_comp));
    MM_HIP(hipMemcpy(&cnt, e->hist_n, sizeof cnt, hipMemcpyDeviceToHost));
    if ((long long)cnt > e->hist_cap)  // reserve_history keeps this from happening
        return fail(MM_ERR_STATE, "mm_sums_history: history overflowed its buffer");
    const long long k = std::min((long long)cnt, max_entries);
    if (k > 0) MM_HIP(hipMemcpy(out, e->hist, sizeof(double) * (size_t)(k * e->na), hipMemcpyDeviceToHost));
    *n = (long long)cnt;
    return MM_OK;
}

int mm_clear_history(mm_engine* e) {
    if (!e) return fail(MM_ERR_INVALID, "mm_clear_history: null");
    MM_TRY(set_device(e));
    MM_HIP(hipStreamSynchronize(e->s_comp));
    MM_HIP(hipMemsetAsync(e->hist_n, 0, sizeof(unsigned long long), e->s_comp));
    MM_HIP(hipStreamSynchronize(e->s_comp));
    e->hist_host = 0;
    return MM_OK;
}

int mm_halo_export_rows(mm_engine* e, int nrows, double* top, double* bottom) {
    if (!e || nrows < 1 || nrows > e->d.h || nrows > mm::kGhost)
        return fail(MM_ERR_INVALID, "mm_halo_export_rows: nrows must be 1..min(h, kGhost)");
    MM_TRY(set_device(e));
    MM_HIP(hipStreamSynchronize(e->s_comm));
    if (top) MM_TRY(copy_rows(e, true, 0, nrows, top));
    if (bottom) MM_TRY(copy_rows(e, true, e->d.h - nrows, nrows, bottom));
    MM_HIP(hipStreamSynchronize(e->s_comp));
    return MM_OK;
}

int mm_halo_import_rows(mm_engine* e, int nrows, const double* top, const double* bottom) {
    if (!e || nrows < 1 || nrows > mm::kGhost)
        return fail(MM_ERR_INVALID, "mm_halo_import_rows: nrows must be 1..kGhost");
    MM_TRY(set_device(e));
    MM_HIP(hipStreamSynchronize(e->s_comm));
    if (top) MM_TRY(copy_rows(e, false, -nrows, nrows, const_cast<double*>(top)));
    if (bottom) MM_TRY(copy_rows(e, false, e->d.h, nrows, const_cast<double*>(bottom)));
    MM_HIP(hipStreamSynchronize(e->s_comp));
    return MM_OK;
}

int mm_halo_export(mm_engine* e, double* top, double* bottom) {
    return mm_halo_export_rows(e, 1, top, bottom);
}

int mm_halo_import(mm_engine* e, const double* top, const double* bottom) {
    return mm_halo_import_rows(e, 1, top, bottom);
}

int mm_debug_read_rows(mm_engine* e, int attr, long long row0, long long nrows, double* host) {
    if (!e || !host || attr < 0 || attr >= e->na || nrows < 0 || row0 < -mm::kGhost ||
        row0 + nrows > e->d.h + mm::kGhost)
        return fail(MM_ERR_INVALID, "mm_debug_read_rows: rows outside the slab + ghost rows");
    MM_TRY(set_device(e));
    MM_HIP(hipStreamSynchronize(e->s_comm));
    MM_HIP(hipMemcpy2DAsync(host, sizeof(double) * e->d.W, e->buf[e->cur][attr] + row0 * e->pitch,
                            sizeof(double) * e->pitch, sizeof(double) * e->d.W, nrows,
                            hipMemcpyDeviceToHost, e->s_comp));
    MM_HIP(hipStreamSynchronize(e->s_comp));
    return MM_OK;
}

int mm_debug_fill_padding(mm_engine* e, double value) {
    if (!e) return fail(MM_ERR_INVALID, "mm_debug_fill_padding: null");
    const long long pad = e->pitch - e->d.W;
    if (pad <= 0) return MM_OK;
    MM_TRY(set_device(e));
    MM_HIP(hipStreamSynchronize(e->s_comm));
    std::vector<double> src((size_t)(pad * e->rows_alloc), value);
    for (int k = 0; k < 2; ++k)
        for (int a = 0; a < e->na; ++a)
            MM_HIP(hipMemcpy2DAsync(e->buf[k][a] - mm::kGhost * e->pitch + e->d.W,
                                    sizeof(double) * e->pitch, src.data(), sizeof(double) * pad,
                                    sizeof(double) * pad, e->rows_alloc, hipMemcpyHostToDevice,
                                    e->s_comp));
    for (int a = 0; a < e->na; ++a)
        if (e->fld_base[a])
            MM_HIP(hipMemcpy2DAsync(e->fld_base[a] + e->d.W, sizeof(double) * e->pitch, src.data(),
                                    sizeof(double) * pad, sizeof(double) * pad, e->rows_alloc,
                                    hipMemcpyHostToDevice, e->s_comp));
    MM_HIP(hipStreamSynchronize(e->s_comp));
    return MM_OK;
}

int mm_set_timing(mm_engine* e, int on) {
    if (!e) return fail(MM_ERR_INVALID, "mm_set_timing: null");
    MM_TRY(set_device(e));
    MM_HIP(hipStreamSynchronize(e->s_comp));
    e->timing = on != 0;
    e->ev_used = 0;
    e->ev_bytes.clear();
    e->timed_launches = 0;
    e->timed_ms = 0.0;
    e->timed_bytes = 0.0;
    return MM_OK;
}

int mm_timing(mm_engine* e, long long* n, double* total_ms, double* bytes_per_launch) {
    if (!e) return fail(MM_ERR_INVALID, "mm_timing: null");
    MM_TRY(set_device(e));
    MM_HIP(hipStreamSynchronize(e->s_comp));
    for (size_t i = 0; i + 1 < e->ev_used; i += 2) {
        float ms = 0.f;
        MM_HIP(hipEventElapsedTime(&ms, e->ev_pool[i], e->ev_pool[i + 1]));
        e->timed_ms += ms;
        e->timed_launches += 1;
        e->timed_bytes += e->ev_bytes[i / 2];
    }
    e->ev_used = 0;
    e->ev_bytes.clear();
    if (n) *n = e->timed_launches;
    if (total_ms) *total_ms = e->timed_ms;
    // algorithmic bytes of a timed launch: each cell of its rows read once and written
    // once per attribute (16 B), whether the launch advances one step or K
    if (bytes_per_launch)
        *bytes_per_launch = e->timed_launches ? e->timed_bytes / (double)e->timed_launches : 0.0;
    return MM_OK;
}

}  // extern "C"
