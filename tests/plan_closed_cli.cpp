// plan_closed_cli.cpp -- the host-only planner (mpi-model_amd/csrc/mm_plan.cpp) on programs
// that hold a closed rate-field diffusion (MM_FLOW_DIFFUSE_CLOSED, mm::PlanIn::closed), for
// tests/test_closed_cpu.py. Built with plain g++ (no ROCm headers). Two things are checked:
//   * a program with a closed diffusion plans one step per pass, field_k == 0, halo depth 1,
//     whatever MM_FIELD_STEPS / MM_FIELD_HALO say and however large the slab is;
//   * every other program plans as it did before the closed kind existed: kTable holds the
//     lines `plan_closed_cli table` printed when built against the planner of the commit
//     before (with -DMM_PLAN_BEFORE_CLOSED, which leaves out what names PlanIn::closed).
// Prints one line per failed check and exits 1, else "ok".
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../mpi-model_amd/csrc/mm_plan.hpp"

namespace {

int g_failed = 0;

void expect(bool ok, const char* what, int line) {
    if (ok) return;
    std::printf("line %d: %s\n", line, what);
    g_failed = 1;
}
#define EXPECT(c) expect((c), #c, __LINE__)

// Slab g of G of an H x W grid (mm_partition_rows), as the engine fills mm::PlanIn.
mm::PlanIn slab(long long H, long long W, int G, int g, int n_attr, bool split) {
    mm::PlanIn in;
    in.H = H, in.W = W, in.nranks = G;
    in.x_init = g * H / G;
    in.h = (g + 1) * H / G - in.x_init;
    in.min_rows = std::min(in.h, H / G);
    in.pitch = (W + mm::kStripCols - 1) / mm::kStripCols * mm::kStripCols;
    in.n_attr = n_attr;
    in.split = split;
    in.knobs.th = 8;
    in.ncu = 256;
    in.slots = [](mm::Kernel kernel, int k, bool) { return kernel == mm::kWide ? 2 : (k > 8 ? 4 : 8); };
    return in;
}

// The programs the engine knew before the closed kind, as sync_program describes them.
enum Program { kDiffuse, kC5, kField, kFieldAlone, kThreePasses };
const char* const kProgramNames[] = {"diffuse", "c5", "field", "field_alone", "three_passes"};

mm::PlanIn program(mm::PlanIn in, Program p, bool halo) {
    in.n_passes = 1;
    switch (p) {
        case kDiffuse:
            in.diffuse_mask = 1;
            break;
        case kC5:
            in.diffuse_mask = 15, in.chains = true, in.ring = true;
            break;
        case kField:  // a field pass on an engine of several attributes: one step per pass
            in.field = true;
            break;
        case kFieldAlone:  // exactly one field diffusion, one attribute: K-step passes
            in.field = true;
            in.field_k = mm::field_k_for(in, halo);
            break;
        case kThreePasses:
            in.n_passes = 3;
            break;
    }
    if (in.n_attr > 1 || in.field || in.chains) in.knobs.th = 8;
    return in;
}

std::string launch_text(const mm::Launch& l) {
    char buf[256];
    std::snprintf(buf, sizeof buf, "%lld-%lld,%lld-%lld s%d th%d/%d x%d n%d w%lld/%lld b%lld", l.lo, l.hi,
                  l.lo2, l.hi2, l.seg, l.th, l.th_edge, l.xcd_remap, l.nstrips, l.waves_a,
                  l.waves_total, l.partial_base);
    return buf;
}

// Everything the engine asks the planner about a program, as one line.
std::string plan_text(const mm::PlanIn& in) {
    std::string s;
    char buf[256];
    const mm::SlabPlan sp = mm::slab_plan(in);
    std::snprintf(buf, sizeof buf, "k%d spl%d rpw%d w%lld sw%d ok%d v%d need%lld |", (int)sp.kernel,
                  sp.steps_per_launch, sp.rows_per_wave, sp.waves_per_pass, sp.seg_waves_per_cu,
                  (int)mm::kstep_ok(in), mm::kernel_variant(in), mm::partials_need(in));
    s += buf;
    for (long long n : {1LL, 7LL, 20LL, 64LL}) {
        s += " [";
        for (int l : mm::pass_lengths(in, n)) s += std::to_string(l) + " ";
        s += "]";
    }
    std::snprintf(buf, sizeof buf, " g%lld/%lld/%lld |", mm::graph_per(in, 20, 0), mm::graph_per(in, 64, 1),
                  mm::graph_per(in, 7, 3, true));
    s += buf;
    for (int k : {1, sp.steps_per_launch})
        for (int red = 0; red < 2; ++red) {
            const mm::PassLaunches p = mm::pass_launches(in, k, red != 0);
            std::snprintf(buf, sizeof buf, " {k%d c%d st%lld d%d sp%d t%lld ", (int)p.kern.kernel,
                          p.kern.cols, p.kern.strips, p.depth, (int)p.split, p.total);
            s += buf + launch_text(p.interior) + " ; " + launch_text(p.border) + "}";
        }
    return s;
}

struct Case {
    long long H, W;
    int G, g, n_attr;
    bool split;
    Program p;
    int field_steps, field_halo;
};

const Case kCases[] = {
    {130, 97, 1, 0, 1, false, kDiffuse, 0, 1},      {2048, 2048, 1, 0, 1, false, kDiffuse, 0, 1},
    {8192, 8192, 1, 0, 1, false, kDiffuse, 0, 1},   {32768, 32768, 1, 0, 1, false, kDiffuse, 4, 4},
    {32768, 32768, 8, 3, 1, true, kDiffuse, 0, 1},  {4096, 4096, 1, 0, 4, false, kC5, 0, 1},
    {67, 300, 3, 1, 4, true, kC5, 4, 4},            {130, 257, 1, 0, 3, false, kField, 4, 4},
    {27, 257, 3, 1, 2, true, kField, 0, 2},         {130, 257, 1, 0, 1, false, kFieldAlone, 0, 1},
    {2048, 2048, 1, 0, 1, false, kFieldAlone, 0, 1}, {8192, 8192, 1, 0, 1, false, kFieldAlone, 3, 1},
    {8192, 8192, 1, 0, 1, true, kFieldAlone, 0, 4}, {8192, 8192, 1, 0, 1, true, kFieldAlone, 4, 1},
    {27, 257, 3, 1, 1, true, kFieldAlone, 4, 4},    {4096, 2048, 2, 1, 1, true, kFieldAlone, 0, 4},
    {130, 97, 1, 0, 3, false, kThreePasses, 4, 4},  {8192, 8192, 2, 0, 2, true, kThreePasses, 0, 1},
};

std::string case_text(const Case& c) {
    mm::PlanIn in = slab(c.H, c.W, c.G, c.g, c.n_attr, c.split);
    in.knobs.field_steps = c.field_steps;
    in.knobs.field_halo = c.field_halo;
    in = program(in, c.p, c.split);
    char buf[128];
    std::snprintf(buf, sizeof buf, "%s %lldx%lld %d/%d na%d fs%d fh%d: ", kProgramNames[c.p], c.H, c.W, c.g,
                  c.G, c.n_attr, c.field_steps, c.field_halo);
    return buf + plan_text(in);
}

// `plan_closed_cli table` of the planner before the closed kind
const char* const kTable[] = {
#include "plan_closed_table.inc"
};

#ifndef MM_PLAN_BEFORE_CLOSED
// A program that holds a closed diffusion: n_passes passes, one of them closed.
void check_closed(mm::PlanIn in, int n_passes, bool halo) {
    in.n_passes = n_passes;
    in.field = in.closed = true;
    in.knobs.th = 8;
    // what the engine computes for a one-attribute, one-pass rate-field program
    in.field_k = mm::field_k_for(in, halo);
    EXPECT(in.field_k == 0);
    EXPECT(!mm::kstep_ok(in) && !mm::passk_ok(in));
    EXPECT(mm::steps_per_launch(in) == 1);
    const mm::SlabPlan sp = mm::slab_plan(in);
    EXPECT(sp.kernel == mm::kOneStep && sp.steps_per_launch == 1 && sp.rows_per_wave == 8);
    EXPECT(sp.waves_per_pass == in.pitch / mm::kStripCols * ((in.h + 7) / 8));
    for (long long n : {1LL, 2LL, 7LL, 20LL, 1000LL}) {
        const std::vector<int> lens = mm::pass_lengths(in, n);
        EXPECT((long long)lens.size() == n && std::all_of(lens.begin(), lens.end(), [](int l) { return l == 1; }));
        EXPECT(mm::next_pass_len(in, n) == 1);
    }
    for (int k = 1; k <= mm::kFieldMaxSteps; ++k) {
        const mm::KernelChoice kc = mm::kernel_for(in, k);
        EXPECT(kc.kernel == mm::kOneStep && kc.cols == 1 && kc.strips == 0);
    }
    for (int red = 0; red < 2; ++red) {
        const mm::PassLaunches p = mm::pass_launches(in, 1, red != 0);
        const long long h = in.h, ns = in.pitch / mm::kStripCols;
        EXPECT(p.kern.kernel == mm::kOneStep && p.depth == 1);
        EXPECT(p.split == (in.split && h >= 3));
        const long long T = p.split ? 1 : 0;
        EXPECT(p.interior.lo == T && p.interior.hi == h - T && p.interior.th == 8 && p.interior.seg == 0);
        EXPECT(p.interior.nstrips == ns && p.interior.waves_total == ns * ((h - 2 * T + 7) / 8));
        if (p.split) {
            EXPECT(p.border.lo == 0 && p.border.hi == 1 && p.border.lo2 == h - 1 && p.border.hi2 == h);
            EXPECT(p.border.th == 1 && p.border.waves_a == ns && p.border.waves_total == 2 * ns);
            EXPECT(p.border.partial_base == p.interior.waves_total);
        }
        EXPECT(p.total == p.interior.waves_total + p.border.waves_total);
        EXPECT(p.total * mm::kMaxAttr <= mm::partials_need(in));
    }
    // the field program at one step per pass plans the same launches: the closed kernel is
    // driven by mm_field_kernel's
    mm::PlanIn f = in;
    f.closed = false;
    f.field_k = 0;
    EXPECT(plan_text(f) == plan_text(in));
    // a forced field_k is ignored too
    in.field_k = 4;
    EXPECT(!mm::kstep_ok(in) && mm::steps_per_launch(in) == 1 && mm::pass_lengths(in, 7).size() == 7);
}
#endif

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "table") == 0) {
        for (const Case& c : kCases) std::printf("\"%s\",\n", case_text(c).c_str());
        return 0;
    }
    const size_t n = sizeof kCases / sizeof kCases[0];
    EXPECT(sizeof kTable / sizeof kTable[0] == n);
    for (size_t i = 0; i < n && i < sizeof kTable / sizeof kTable[0]; ++i)
        if (case_text(kCases[i]) != kTable[i]) {
            std::printf("plan changed:\n  was %s\n  is  %s\n", kTable[i], case_text(kCases[i]).c_str());
            g_failed = 1;
        }
#ifndef MM_PLAN_BEFORE_CLOSED
    EXPECT(!mm::PlanIn().closed);
    // 2^22 cells is where a lone field diffusion starts to fuse 4 steps per pass
    const long long shapes[][2] = {{130, 97}, {27, 257}, {2048, 2048}, {4096, 2048}, {8192, 8192}, {4096, 32768}};
    for (const auto& s : shapes)
        for (int fs : {0, 4})
            for (int fh : {1, 4})
                for (int halo = 0; halo < 2; ++halo)
                    for (int passes : {1, 3}) {
                        mm::PlanIn in = slab(s[0], s[1], 1, 0, 1, halo != 0);
                        in.knobs.field_steps = fs;
                        in.knobs.field_halo = fh;
                        if (s[0] * s[1] >= (1LL << 22) && passes == 1) {  // the field kind would fuse here
                            mm::PlanIn f = in;
                            f.n_passes = 1, f.field = true;
                            EXPECT((mm::field_k_for(f, halo != 0) >= 2) == (!halo || fh == 4));
                        }
                        check_closed(in, passes, halo != 0);
                    }
    // chains: every slab, several attributes
    for (int g = 0; g < 3; ++g)
        for (int na : {1, 3}) {
            mm::PlanIn in = slab(27, 257, 3, g, na, true);
            in.knobs.field_steps = in.knobs.field_halo = 4;
            check_closed(in, 1, true);
        }
    for (int g = 0; g < 2; ++g) {
        mm::PlanIn in = slab(8192, 8192, 2, g, 1, true);
        in.knobs.field_steps = in.knobs.field_halo = 4;
        check_closed(in, 1, true);
        in = slab(16, 257, 2, g, 1, true);
        check_closed(in, 1, true);
    }
#endif
    if (!g_failed) std::printf("ok\n");
    return g_failed;
}
