// plan_field_cli.cpp -- the host-only planner (mpi-model_amd/csrc/mm_plan.cpp) on programs
// with a rate-field pass (mm::PlanIn::field), for tests/test_ratefield_cpu.py. Built with
// plain g++ (no ROCm headers). Prints one line per failed check and exits 1, else "ok".
#include <algorithm>
#include <cstdio>
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

// Slab g of G of an H x W grid (mm_partition_rows), one attribute, a one-pass program.
mm::PlanIn slab(long long H, long long W, int G, int g) {
    mm::PlanIn in;
    in.H = H, in.W = W, in.nranks = G;
    in.x_init = g * H / G;
    in.h = (g + 1) * H / G - in.x_init;
    in.min_rows = std::min(in.h, H / G);
    in.pitch = (W + mm::kStripCols - 1) / mm::kStripCols * mm::kStripCols;
    in.n_attr = 1, in.n_passes = 1, in.diffuse_mask = 1;
    in.split = G > 1;
    in.ncu = 256;
    in.slots = [](mm::Kernel, int, bool) { return 8; };
    return in;
}

bool same_launch(const mm::Launch& a, const mm::Launch& b) {
    return a.lo == b.lo && a.hi == b.hi && a.lo2 == b.lo2 && a.hi2 == b.hi2 && a.seg == b.seg &&
           a.th == b.th && a.th_edge == b.th_edge && a.xcd_remap == b.xcd_remap &&
           a.nstrips == b.nstrips && a.waves_a == b.waves_a && a.waves_total == b.waves_total &&
           a.partial_base == b.partial_base;
}

bool same_plan(const mm::PlanIn& a, const mm::PlanIn& b) {
    bool same = mm::passk_ok(a) == mm::passk_ok(b) &&
                mm::steps_per_launch(a) == mm::steps_per_launch(b) &&
                mm::partials_need(a) == mm::partials_need(b) &&
                mm::kernel_variant(a) == mm::kernel_variant(b);
    for (long long n : {1LL, 7LL, 20LL, 64LL, 1000LL}) {
        same = same && mm::pass_lengths(a, n) == mm::pass_lengths(b, n);
        for (long long re : {0LL, 1LL, 3LL})
            same = same && mm::graph_per(a, n, re) == mm::graph_per(b, n, re) &&
                   mm::graph_per(a, n, re, true) == mm::graph_per(b, n, re, true);
    }
    const mm::SlabPlan sa = mm::slab_plan(a), sb = mm::slab_plan(b);
    same = same && sa.kernel == sb.kernel && sa.steps_per_launch == sb.steps_per_launch &&
           sa.rows_per_wave == sb.rows_per_wave && sa.waves_per_pass == sb.waves_per_pass &&
           sa.seg_waves_per_cu == sb.seg_waves_per_cu;
    for (int k = 1; k <= mm::steps_per_launch(a); ++k)
        for (int red = 0; red < 2; ++red) {
            const mm::KernelChoice ka = mm::kernel_for(a, k), kb = mm::kernel_for(b, k);
            same = same && ka.kernel == kb.kernel && ka.cols == kb.cols && ka.strips == kb.strips;
            const mm::PassLaunches pa = mm::pass_launches(a, k, red), pb = mm::pass_launches(b, k, red);
            same = same && pa.depth == pb.depth && pa.split == pb.split && pa.total == pb.total &&
                   same_launch(pa.interior, pb.interior) && same_launch(pa.border, pb.border);
        }
    return same;
}

}  // namespace

int main() {
    const long long shapes[][4] = {{512, 512, 1, 0},   {8192, 8192, 1, 0}, {300, 700, 2, 1},
                                   {77, 300, 4, 2},    {27, 257, 3, 0},    {16, 130, 8, 7},
                                   {32768, 32768, 8, 3}};
    for (const auto& s : shapes) {
        const mm::PlanIn base = slab(s[0], s[1], (int)s[2], (int)s[3]);

        // field = false: exactly the plan of a PlanIn that never heard of the flag, and for
        // this one-diffusion program that is a K-step plan
        mm::PlanIn off = base;
        off.field = false;
        EXPECT(mm::passk_ok(base));
        EXPECT(same_plan(off, base));

        // field = true: one step per pass on the one-step schedule
        mm::PlanIn on = base;
        on.field = true;
        on.diffuse_mask = 0;  // a rate-field pass holds no uniform diffusion
        EXPECT(!mm::passk_ok(on));
        EXPECT(mm::steps_per_launch(on) == 1);
        EXPECT(mm::pass_lengths(on, 7) == std::vector<int>(7, 1));
        EXPECT(mm::next_pass_len(on, 20) == 1);
        EXPECT(mm::kernel_for(on, 1).kernel == mm::kOneStep);
        EXPECT(mm::slab_plan(on).kernel == mm::kOneStep);
        EXPECT(mm::slab_plan(on).steps_per_launch == 1);
        for (int red = 0; red < 2; ++red) {
            const mm::PassLaunches p = mm::pass_launches(on, 1, red);
            EXPECT(p.kern.kernel == mm::kOneStep);
            EXPECT(p.depth == 1);
            const long long h = on.h, ns = on.pitch / mm::kStripCols;
            EXPECT(p.interior.nstrips == ns);
            EXPECT(p.interior.th == 8);
            if (on.split && h >= 3) {
                // the border launch: one row on each side, one row per wave, its partials
                // behind the interior's
                EXPECT(p.split);
                EXPECT(p.interior.lo == 1 && p.interior.hi == h - 1);
                EXPECT(p.border.lo == 0 && p.border.hi == 1);
                EXPECT(p.border.lo2 == h - 1 && p.border.hi2 == h);
                EXPECT(p.border.th == 1);
                EXPECT(p.border.waves_a == ns && p.border.waves_total == 2 * ns);
                EXPECT(p.border.partial_base == p.interior.waves_total);
            } else {
                EXPECT(!p.split);
                EXPECT(p.interior.lo == 0 && p.interior.hi == h);
                EXPECT(p.border.waves_total == 0);
            }
            EXPECT(p.interior.waves_total == ns * ((p.interior.hi - p.interior.lo + 7) / 8));
            EXPECT(p.total == p.interior.waves_total + p.border.waves_total);
            EXPECT(p.total * mm::kMaxAttr <= mm::partials_need(on));
        }
        // a graph holds an even number of buffer flips: two one-pass steps at least
        EXPECT(mm::graph_per(on, 64, 0) > 0 && mm::graph_per(on, 64, 0) % 2 == 0);
    }
    if (!g_failed) std::printf("ok\n");
    return g_failed;
}
