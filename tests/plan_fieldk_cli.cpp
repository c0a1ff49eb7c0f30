// plan_fieldk_cli.cpp -- the host-only planner (mpi-model_amd/csrc/mm_plan.cpp) on programs
// whose rate-field passes fuse K steps (mm::PlanIn::field_k, mm_fieldk_kernel), for
// tests/test_fieldk_cpu.py. Built with plain g++ (no ROCm headers). Prints one line per
// failed check and exits 1, else "ok <kFieldMaxSteps>".
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "plan_test.hpp"

namespace {

// Slab g of G of an H x W grid, one attribute, the program one rate-field diffusion, 8 slots
// per CU whatever the kernel. field_k is left to the checks, which set it themselves.
mm::PlanIn slab(long long H, long long W, int G, int g) {
    mm::PlanIn in = with_flows(slab(H, W, G, g, 1, G > 1), {F(0)}, G > 1);
    EXPECT(in.field && in.n_passes == 1 && in.diffuse_mask == 0 && in.knobs.th == 8);
    in.field_k = 0;
    in.slots = [](mm::Kernel, int, bool) { return 8; };
    return in;
}

void check_on(const mm::PlanIn& base, int K) {
    mm::PlanIn in = base;
    in.field_k = K;
    EXPECT(!mm::passk_ok(in) && mm::kstep_ok(in));
    EXPECT(mm::steps_per_launch(in) == K);
    for (long long n : {1LL, 7LL, 20LL, 64LL, 1000LL}) {
        const std::vector<int> lens = mm::pass_lengths(in, n);
        long long sum = 0;
        int lo = K, hi = 0;
        for (int l : lens) {
            sum += l;
            lo = std::min(lo, l), hi = std::max(hi, l);
        }
        EXPECT(sum == n);
        EXPECT(hi <= K && lo >= 1 && hi - lo <= 1);
        EXPECT((long long)lens.size() == ceil_div(n, K));
        EXPECT(mm::next_pass_len(in, n) == lens[0]);
    }
    const mm::KernelChoice one = mm::kernel_for(in, 1);
    EXPECT(one.kernel == mm::kOneStep && one.cols == 1 && one.strips == 0);
    for (int k = 2; k <= K; ++k) {
        const mm::KernelChoice kc = mm::kernel_for(in, k);
        EXPECT(kc.kernel == mm::kFieldK && kc.cols == 2);
        EXPECT(kc.strips == ceil_div(in.W, mm::passk_out_cols(k)));
    }
    for (int k = 1; k <= K; ++k)
        for (int red = 0; red < 2; ++red) {
            const mm::PassLaunches p = mm::pass_launches(in, k, red);
            EXPECT(!p.split && p.depth == k);
            EXPECT(p.interior.lo == 0 && p.interior.hi == in.h);
            EXPECT(p.interior.lo2 == p.interior.hi2 && p.border.waves_total == 0);
            EXPECT(p.total == p.interior.waves_total && p.interior.partial_base == 0);
            EXPECT(p.total * mm::kMaxAttr <= mm::partials_need(in));
            EXPECT(p.total * k <= mm::partials_need(in));
            if (k == 1) continue;
            // segments: even, at least 16 rows, offsets into state and field below 2^31, and
            // the count mm_passk.hpp's seg_map gives for full-length edge segments
            const mm::Launch& l = p.interior;
            EXPECT(l.seg == 1 && l.xcd_remap == 0 && l.nstrips == p.kern.strips);
            EXPECT(l.th >= 16 && l.th % 2 == 0 && l.th_edge == l.th);
            EXPECT(l.th <= mm::fieldk_max_rows(k, in.pitch));
            EXPECT((l.th + 3 * k + 2 * mm::field_ring(k)) * in.pitch * 8 < (1LL << 31));
            EXPECT(l.waves_total == mm::seg_wave_count(in.h, l.nstrips, l.th, l.th_edge));
            EXPECT(l.waves_total == l.nstrips * ceil_div(in.h, l.th) && l.waves_a == l.waves_total);
        }
    const mm::SlabPlan sp = mm::slab_plan(in);
    EXPECT(sp.kernel == mm::kFieldK && sp.steps_per_launch == K);
    EXPECT(sp.rows_per_wave == mm::pass_launches(in, K, false).interior.th);
    EXPECT(sp.waves_per_pass == mm::pass_launches(in, K, false).total);
    // one flip per pass: a graph of whole K-step passes with an even number of them
    const long long per = mm::graph_per(in, 64, 0);
    EXPECT(per > 0 && 64 % per == 0);
    EXPECT(mm::pass_lengths(in, per).size() % 2 == 0);
    EXPECT(mm::graph_per(in, 64, 1) > 0);
}

}  // namespace

int main() {
    // MM_FIELD_STEPS: 0 / unset auto, 1 off, 2..kFieldMaxSteps that K; anything else is ignored
    EXPECT(mm::Knobs().field_steps == 0);
    EXPECT(knobs_of("MM_FIELD_STEPS", "0").field_steps == 0);
    EXPECT(knobs_of("MM_FIELD_STEPS", "1").field_steps == 1);
    for (int k = 2; k <= mm::kFieldMaxSteps; ++k)
        EXPECT(knobs_of("MM_FIELD_STEPS", std::to_string(k).c_str()).field_steps == k);
    EXPECT(knobs_of("MM_FIELD_STEPS", std::to_string(mm::kFieldMaxSteps + 1).c_str()).field_steps == 0);
    EXPECT(knobs_of("MM_FIELD_STEPS", "-3").field_steps == 0);
    EXPECT(knobs_of("MM_STEPS_PER_PASS", "4").field_steps == 0);
    EXPECT(mm::kFieldMaxSteps >= 4 && mm::kFieldK == 4);

    // field_k = 0 on the shapes of plan_field_cli.cpp: today's one-step plans
    const long long shapes[][4] = {{512, 512, 1, 0},   {8192, 8192, 1, 0}, {300, 700, 2, 1},
                                   {77, 300, 4, 2},    {27, 257, 3, 0},    {16, 130, 8, 7},
                                   {32768, 32768, 8, 3}};
    for (const auto& s : shapes) {
        mm::PlanIn on = slab(s[0], s[1], (int)s[2], (int)s[3]);
        check_one_step(on);
        on.knobs.field_steps = 4;  // the knob alone changes no plan: the engine sets field_k
        check_one_step(on);
    }

    // what the engine asks before it sets field_k
    {
        mm::PlanIn in = slab(64, 130, 1, 0);
        EXPECT(mm::field_steps_for(in) == 0);  // auto: small grids keep one step per pass
        in.h = in.H = 255, in.W = 257;         // 65535 cells: below 2^16 whatever the table says
        EXPECT(mm::field_steps_for(in) == 0);
        in = slab(64, 130, 1, 0);
        for (int k = 2; k <= mm::kFieldMaxSteps; ++k) {
            in.knobs.field_steps = k;
            EXPECT(mm::field_steps_for(in) == k);
        }
        in.knobs.field_steps = 1;
        EXPECT(mm::field_steps_for(in) == 0);
        in.knobs.field_steps = 4;
        in.knobs.passk = false;  // MM_PASSK=0: one step per kernel pass
        EXPECT(mm::field_steps_for(in) == 0);
        mm::PlanIn big = slab(32768, 32768, 1, 0);
        big.knobs.field_steps = 1;
        EXPECT(mm::field_steps_for(big) == 0);
        big.knobs.field_steps = 0;
        const int k = mm::field_steps_for(big);
        EXPECT(k == 0 || (k >= 2 && k <= mm::kFieldMaxSteps));
    }

    const long long grids[][2] = {{512, 512}, {8192, 8192}, {50, 257}, {3, 130}};
    for (const auto& g : grids)
        for (int K = 2; K <= mm::kFieldMaxSteps; ++K) check_on(slab(g[0], g[1], 1, 0), K);
    // a tall, narrow grid: the occupancy plan's segments stay far below the 2^31 offset cap
    {
        mm::PlanIn in = slab(300000, 5000, 1, 0);
        check_on(in, mm::kFieldMaxSteps);
        in.field_k = mm::kFieldMaxSteps;
        const int th = mm::pass_launches(in, in.field_k, false).interior.th;
        EXPECT(th >= 16 && th < mm::fieldk_max_rows(in.field_k, in.pitch) / 4);
    }
    // where the cap binds: 65536^2 under the default knobs, and the grid of
    // tests/test_gpu_field_large.py (8200 x 32768, MM_SEG_WAVES=0.001: one segment of the cap
    // and the rest per strip)
    for (int K = 2; K <= mm::kFieldMaxSteps; ++K) {
        mm::PlanIn big = slab(65536, 65536, 1, 0);
        mm::PlanIn cap = slab(8200, 32768, 1, 0);
        cap.knobs = knobs_of("MM_SEG_WAVES", "0.001");
        cap.knobs.th = 8;
        for (mm::PlanIn* in : {&big, &cap}) {
            check_on(*in, K);
            in->field_k = K;
            for (int k = 2; k <= K; ++k)
                for (int red = 0; red < 2; ++red) {
                    const long long maxr = mm::fieldk_max_rows(k, in->pitch);
                    const mm::Launch l = mm::pass_launches(*in, k, red).interior;
                    EXPECT(l.th == (maxr & ~1LL) && l.th_edge == l.th);
                    EXPECT(maxr == (1LL << 31) / (in->pitch * 8) - (3 * k + 2 * mm::field_ring(k) + 8));
                    EXPECT(l.waves_total == l.nstrips * ceil_div(in->h, l.th));
                }
            EXPECT(mm::slab_plan(*in).rows_per_wave == (mm::fieldk_max_rows(K, in->pitch) & ~1LL));
        }
        // 8200 rows: two segments per strip, the second of 8200 - cap rows ends at the last row
        const long long th = mm::slab_plan(cap).rows_per_wave;
        EXPECT(th < 8200 && 8200 - th >= 16 && 8200 - th <= 92 && ceil_div(8200, th) == 2);
    }
    EXPECT(mm::fieldk_max_rows(4, 32768) == 8140 && mm::fieldk_max_rows(2, 32768) == 8146);
    EXPECT(mm::fieldk_max_rows(4, 65536) == 4044);

    // the auto rule and the non-temporal-store rule at the shapes the GPU tests rely on
    {
        mm::PlanIn in = slab(2048, 2048, 1, 0);
        EXPECT(mm::field_steps_for(in) == 4 && mm::kernel_variant(in) == 0);
        EXPECT(mm::field_steps_for(slab(2047, 2048, 1, 0)) == 0);
        EXPECT(mm::kernel_variant(slab(4096, 4096, 1, 0)) == 0);  // exactly 256 MiB: not above
        in = slab(4104, 4096, 1, 0);
        EXPECT(mm::field_steps_for(in) == 4 && mm::kernel_variant(in) == 1);
        // the plans of those two grids with 8 slots per CU: 16-row segments in 18 strips,
        // 36-row segments in 35 strips (114 segment rows)
        in.field_k = 4;
        mm::Launch l = mm::pass_launches(in, 4, false).interior;
        EXPECT(l.th == 36 && l.nstrips == 35 && ceil_div(in.h, l.th) == 114);
        EXPECT(mm::pass_lengths(in, 7) == (std::vector<int>{4, 3}));
        in = slab(2048, 2048, 1, 0);
        in.field_k = 4;
        l = mm::pass_launches(in, 4, false).interior;
        EXPECT(l.th == 16 && l.nstrips == 18);
        EXPECT(mm::pass_lengths(in, 7) == (std::vector<int>{4, 3}));
        // MM_KERNEL_VARIANT overrides the size rule both ways
        in.knobs = knobs_of("MM_KERNEL_VARIANT", "1");
        EXPECT(mm::kernel_variant(in) == 1);
        in = slab(4104, 4096, 1, 0);
        in.knobs = knobs_of("MM_KERNEL_VARIANT", "0");
        EXPECT(mm::kernel_variant(in) == 0);
    }

    if (!g_failed) std::printf("ok %d\n", mm::kFieldMaxSteps);
    return g_failed;
}
