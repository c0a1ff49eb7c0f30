// plan_field_cli.cpp -- the host-only planner (mpi-model_amd/csrc/mm_plan.cpp) on programs
// with a rate-field pass (mm::PlanIn::field), for tests/test_ratefield_cpu.py. Built with
// plain g++ (no ROCm headers). Prints one line per failed check and exits 1, else "ok".
#include <algorithm>
#include <vector>

#include "plan_test.hpp"

namespace {

// Slab g of G of an H x W grid, one attribute, the program one uniform diffusion, 8 slots per
// CU whatever the kernel.
mm::PlanIn slab(long long H, long long W, int G, int g) {
    mm::PlanIn in = with_flows(slab(H, W, G, g, 1, G > 1), {D(0)}, G > 1);
    in.slots = [](mm::Kernel, int, bool) { return 8; };
    return in;
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
                   launch_text(pa.interior) == launch_text(pb.interior) &&
                   launch_text(pa.border) == launch_text(pb.border);
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
        mm::PlanIn on = with_flows(base, {F(0)}, s[2] > 1);
        EXPECT(on.field && on.diffuse_mask == 0);  // a rate-field pass holds no uniform diffusion
        on.field_k = 0;  // (the K-step plans: plan_fieldk_cli.cpp)
        check_one_step(on);
    }
    if (!g_failed) std::printf("ok\n");
    return g_failed;
}
