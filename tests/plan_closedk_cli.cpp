// plan_closedk_cli.cpp -- the host-only planner (mpi-model_amd/csrc/mm_plan.cpp) on K-step
// passes of the closed rate-field diffusion (MM_CLOSED_STEPS, mm::PlanIn::closed_k,
// mm::kClosedK), for tests/test_closedk_cpu.py. Built with plain g++ (no ROCm headers).
//   * With the knob unset every program of tests/plan_closed_table.inc prints the line it
//     printed before the knob existed (the cases and the line format are
//     tests/plan_closed_cli.cpp's), and a closed program plans one step per pass.
//   * With MM_CLOSED_STEPS=K a program that is one closed diffusion of one attribute on a slab
//     without a halo plans kernel 5 over ceil(W / closedk_out_cols(K)) strips in balanced
//     passes; a pass of one step stays on the one-step kernel.
//   * closed_k_for is 0 with a halo, under MM_PASSK=0 and at a pitch whose closedk_max_rows is
//     under 64; the engine's conditions (one attribute, exactly one closed diffusion) are
//     mm::set_program's, asked through real flow lists; a knob value above the maximum clamps.
//   * closedk_max_rows keeps every row the kernel addresses below 2^31 bytes.
// Prints one line per failed check and exits 1, else "ok"; `plan_closedk_cli max` prints
// kClosedMaxSteps.
#include <algorithm>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "plan_closed_cases.hpp"

namespace {

// A one-attribute slab without a halo whose program is one closed diffusion.
mm::PlanIn closed_alone(long long H, long long W, const std::map<std::string, std::string>& env) {
    mm::PlanIn in = slab(H, W, 1, 0, 1, false);
    in.knobs = knobs_of(env);
    in = with_flows(in, {C(0)}, false);
    EXPECT(in.n_passes == 1 && in.field && in.closed && in.knobs.th == 8);
    return in;
}

// closed_k of slab `in` (its knobs set) under the program of `flows`.
int closed_k_with(const mm::PlanIn& in, const std::vector<mm::Flow>& flows, bool halo) {
    return with_flows(in, flows, halo).closed_k;
}

void check_off(const mm::PlanIn& in) {
    EXPECT(in.closed_k == 0 && in.field_k == 0);
    EXPECT(!mm::kstep_ok(in) && mm::steps_per_launch(in) == 1);
    EXPECT(mm::slab_plan(in).kernel == mm::kOneStep);
    EXPECT(mm::pass_lengths(in, 7) == std::vector<int>(7, 1));
    for (int k = 1; k <= mm::kClosedMaxSteps; ++k) EXPECT(mm::kernel_for(in, k).kernel == mm::kOneStep);
}

void check_on(long long H, long long W, int K) {
    const mm::PlanIn in = closed_alone(H, W, {{"MM_CLOSED_STEPS", std::to_string(K)}});
    EXPECT(in.closed_k == K && in.field_k == 0);
    EXPECT(mm::kstep_ok(in) && !mm::passk_ok(in) && mm::steps_per_launch(in) == K);
    const long long ns = (W + mm::closedk_out_cols(K) - 1) / mm::closedk_out_cols(K);
    for (int k = 2; k <= K; ++k) {
        const mm::KernelChoice kc = mm::kernel_for(in, k);
        const long long nsk = (W + mm::closedk_out_cols(k) - 1) / mm::closedk_out_cols(k);
        EXPECT(kc.kernel == mm::kClosedK && (int)kc.kernel == 5 && kc.cols == 2 && kc.strips == nsk);
    }
    const mm::KernelChoice k1 = mm::kernel_for(in, 1);
    EXPECT(k1.kernel == mm::kOneStep && k1.cols == 1 && k1.strips == 0);
    // ceil(n / K) balanced passes
    for (long long n : {1LL, 2LL, 7LL, 20LL, 64LL, 1001LL}) {
        const std::vector<int> lens = mm::pass_lengths(in, n);
        long long sum = 0;
        for (int l : lens) sum += l;
        EXPECT(sum == n && (long long)lens.size() == (n + K - 1) / K);
        EXPECT(*std::max_element(lens.begin(), lens.end()) - *std::min_element(lens.begin(), lens.end()) <= 1);
        EXPECT(std::is_sorted(lens.rbegin(), lens.rend()));
    }
    if (K == 2) EXPECT(mm::pass_lengths(in, 7) == (std::vector<int>{2, 2, 2, 1}));
    if (K == 3) EXPECT(mm::pass_lengths(in, 7) == (std::vector<int>{3, 2, 2}));
    if (K == 4) EXPECT(mm::pass_lengths(in, 7) == (std::vector<int>{4, 3}));
    const mm::SlabPlan sp = mm::slab_plan(in);
    EXPECT(sp.kernel == mm::kClosedK && sp.steps_per_launch == K && sp.rows_per_wave >= 16);
    EXPECT(sp.rows_per_wave <= std::max<long long>(16, mm::closedk_max_rows(K, in.pitch)));
    EXPECT(sp.seg_waves_per_cu == in.slots(mm::kClosedK, K, false));
    for (int red = 0; red < 2; ++red) {
        const mm::PassLaunches p = mm::pass_launches(in, K, red != 0);
        EXPECT(p.kern.kernel == mm::kClosedK && p.depth == K && !p.split);
        EXPECT(p.interior.lo == 0 && p.interior.hi == H && p.interior.seg == 1 && p.interior.nstrips == ns);
        EXPECT(p.interior.th == p.interior.th_edge);  // edge ratio 1.0
        EXPECT(p.interior.waves_total == mm::seg_wave_count(H, ns, p.interior.th, p.interior.th_edge));
        EXPECT(p.interior.waves_total == sp.waves_per_pass && p.border.waves_total == 0);
        EXPECT(p.total == p.interior.waves_total);
        EXPECT(p.total * mm::kClosedMaxSteps <= mm::partials_need(in));
        // a pass of one step is mm_closed_kernel's launch, as with the knob unset
        const mm::PassLaunches one = mm::pass_launches(in, 1, red != 0);
        const mm::PassLaunches was = mm::pass_launches(closed_alone(H, W, {}), 1, red != 0);
        EXPECT(one.kern.kernel == mm::kOneStep && one.depth == 1 && one.interior.seg == 0);
        EXPECT(launch_text(one.interior) == launch_text(was.interior) && one.total == was.total);
    }
    // a graph holds whole passes and an even number of flips
    EXPECT(mm::graph_per(in, 64 * K, 0) % (2 * K) == 0);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "max") == 0) {
        std::printf("%d\n", mm::kClosedMaxSteps);
        return 0;
    }
    // the knob unset: the table of the planner before the closed kind, line for line
    check_table();
    // ... and with the knob set, which no program of the table reads
    check_table(mm::kClosedMaxSteps);
    for (const Case& c : kCases) EXPECT(case_in(c, mm::kClosedMaxSteps).closed_k == 0);
    // defaults mean "off"
    EXPECT(mm::Knobs().closed_steps == 0 && mm::PlanIn().closed_k == 0);
    EXPECT(mm::kClosedMaxSteps >= 2 && (int)mm::kClosedK == 5);
    // the knob: 0, 1, unset and junk are one step per pass; above the maximum clamps
    EXPECT(knobs_of({}).closed_steps == 0);
    EXPECT(knobs_of({{"MM_CLOSED_STEPS", "0"}}).closed_steps == 0);
    EXPECT(knobs_of({{"MM_CLOSED_STEPS", "1"}}).closed_steps == 1);
    EXPECT(knobs_of({{"MM_CLOSED_STEPS", "-3"}}).closed_steps == 0);
    EXPECT(knobs_of({{"MM_CLOSED_STEPS", "x"}}).closed_steps == 0);
    EXPECT(knobs_of({{"MM_CLOSED_STEPS", "2"}}).closed_steps == 2);
    EXPECT(knobs_of({{"MM_CLOSED_STEPS", "99"}}).closed_steps == mm::kClosedMaxSteps);
    EXPECT(knobs_of({{"MM_CLOSED_STEPS", "99999999999999"}}).closed_steps == mm::kClosedMaxSteps);
    EXPECT(knobs_of({{"MM_CLOSED_STEPS", "3"}}).field_steps == 0);
    EXPECT(knobs_of({{"MM_FIELD_STEPS", "3"}}).closed_steps == 0);

    const long long shapes[][2] = {{1, 1}, {13, 6}, {27, 257}, {130, 97}, {50, 257}, {2048, 2048}, {8192, 8192}, {8200, 32768}};
    for (const auto& s : shapes) {
        check_off(closed_alone(s[0], s[1], {}));
        check_off(closed_alone(s[0], s[1], {{"MM_CLOSED_STEPS", "1"}}));
        check_off(closed_alone(s[0], s[1], {{"MM_CLOSED_STEPS", "0"}}));
        // MM_FIELD_STEPS / MM_FIELD_HALO have no effect on a closed program
        check_off(closed_alone(s[0], s[1], {{"MM_FIELD_STEPS", "4"}, {"MM_FIELD_HALO", "4"}}));
        check_off(closed_alone(s[0], s[1], {{"MM_CLOSED_STEPS", "4"}, {"MM_PASSK", "0"}}));
        for (int K = 2; K <= mm::kClosedMaxSteps; ++K) {
            check_on(s[0], s[1], K);
            const std::string ks = std::to_string(K);
            const mm::PlanIn a = closed_alone(s[0], s[1], {{"MM_CLOSED_STEPS", ks}});
            const mm::PlanIn b = closed_alone(s[0], s[1], {{"MM_CLOSED_STEPS", ks}, {"MM_FIELD_STEPS", "2"}, {"MM_FIELD_HALO", "3"}});
            EXPECT(plan_text(a) == plan_text(b));
        }
        EXPECT(closed_alone(s[0], s[1], {{"MM_CLOSED_STEPS", "77"}}).closed_k == mm::kClosedMaxSteps);
    }
    // where closed_k_for is 0
    {
        const std::map<std::string, std::string> on = {{"MM_CLOSED_STEPS", "3"}};
        mm::PlanIn in = closed_alone(130, 257, on);
        EXPECT(mm::closed_k_for(in, false) == 3);
        EXPECT(mm::closed_k_for(in, true) == 0);   // a halo: a chain, any halo mode, MM_SELF_HALO
        EXPECT(closed_k_with(in, {C(0)}, false) == 3);
        EXPECT(closed_k_with(in, {T(0, -1), C(0)}, false) == 0);
        EXPECT(closed_k_with(in, {C(0), C(0)}, false) == 0);
        mm::PlanIn two = in;
        two.n_attr = 2;
        EXPECT(closed_k_with(two, {C(0)}, false) == 0);  // two attributes
        mm::PlanIn open = in;
        open.closed = false;  // a field program is not a closed one
        EXPECT(mm::closed_k_for(open, false) == 0);
        mm::PlanIn off = in;
        off.knobs.passk = false;
        EXPECT(mm::closed_k_for(off, false) == 0);
        // a chain's slabs, and one slab with a halo
        for (int g = 0; g < 3; ++g) {
            mm::PlanIn c = slab(27, 257, 3, g, 1, true);
            c.knobs = knobs_of({{"MM_CLOSED_STEPS", "4"}, {"MM_FIELD_HALO", "2"}});
            c = with_flows(c, {C(0)}, true);
            EXPECT(c.closed && mm::field_k_for(c, true) == 0);
            check_off(c);
        }
        // a pitch whose closedk_max_rows is under 64
        mm::PlanIn wide = in;
        wide.pitch = 1LL << 22;
        EXPECT(mm::closedk_max_rows(mm::kClosedMaxSteps, wide.pitch) < 64 && mm::closed_k_for(wide, false) == 0);
        wide.pitch = 1LL << 21;
        EXPECT(mm::closedk_max_rows(mm::kClosedMaxSteps, wide.pitch) >= 64 && mm::closed_k_for(wide, false) == 3);
        // a closed_k the engine did not set for a closed program is ignored
        mm::PlanIn stray = closed_alone(130, 257, {});
        stray.closed = false, stray.closed_k = 3;
        EXPECT(!mm::kstep_ok(stray) && mm::steps_per_launch(stray) == 1);
    }
    // geometry: the halo the design needs, the ring, and the 2^31 cap
    for (int K = 2; K <= mm::kClosedMaxSteps; ++K) {
        const int oc = mm::closedk_out_cols(K);
        EXPECT((mm::kStripCols - oc) % 4 == 0 && (mm::kStripCols - oc) / 2 >= K + 1 && oc >= 64);
        const int ring = mm::closed_ring(K);
        EXPECT(ring % mm::kFieldPrefetch == 0 && ring >= mm::kFieldPrefetch + 2 * (K - 1) + 1);
        EXPECT(ring >= mm::field_ring(K) && 3 * K - 1 <= ring);
        for (long long pitch : {128LL, 384LL, 8192LL, 32768LL, 1LL << 20}) {
            const long long rows = mm::closedk_max_rows(K, pitch);
            EXPECT(rows >= 64 && rows < mm::fieldk_max_rows(K, pitch));
            // the deepest rows a wave addresses (mm_closedk.hpp closedk_segment): the loop runs
            // 3K - 1 iterations and the rows rounded up to a ring; the state is loaded
            // kFieldPrefetch rows ahead of the iteration, the field a ring ahead of level K's
            // row, whose range starts one row above the state's; and the lane's column offset
            const long long iters = 3 * K - 1 + (rows + ring - 1) / ring * ring;
            const long long v_row = iters - 1 + mm::kFieldPrefetch;
            const long long f_row = iters - 1 - 2 * (K - 1) + 1 + ring;
            EXPECT((std::max(v_row, f_row) + 1) * pitch * 8 + pitch * 8 < (1LL << 31));
            EXPECT((rows + 2 * K + 2) * pitch * 8 < (1LL << 31));  // the field's range in bytes
        }
    }
    if (!g_failed) std::printf("ok\n");
    return g_failed;
}
