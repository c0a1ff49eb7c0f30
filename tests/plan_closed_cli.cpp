// plan_closed_cli.cpp -- the host-only planner (mpi-model_amd/csrc/mm_plan.cpp) on programs
// that hold a closed rate-field diffusion (MM_FLOW_DIFFUSE_CLOSED, mm::PlanIn::closed), for
// tests/test_closed_cpu.py. Built with plain g++ (no ROCm headers). Two things are checked:
//   * a program with a closed diffusion plans one step per pass, field_k == 0, halo depth 1,
//     whatever MM_FIELD_STEPS / MM_FIELD_HALO say and however large the slab is;
//   * every other program plans as it did before the closed kind existed: kTable holds the
//     lines `plan_closed_cli table` printed when built against the planner of the commit
//     before (tests/plan_closed_cases.hpp).
// Prints one line per failed check and exits 1, else "ok".
#include <algorithm>
#include <cstring>
#include <vector>

#include "plan_closed_cases.hpp"

namespace {

// A program that holds a closed diffusion: n_passes passes, one of them closed.
void check_closed(mm::PlanIn in, int n_passes, bool halo) {
    const std::vector<mm::Flow> one = {C(0)}, three = {D(0), C(0), D(0)};
    in = with_flows(in, n_passes == 1 ? one : three, halo);
    EXPECT(in.n_passes == n_passes && in.field && in.closed && in.knobs.th == 8);
    // a lone closed diffusion is no lone field diffusion, and field_k_for refuses it too
    EXPECT(in.field_k == 0 && mm::field_k_for(in, halo) == 0);
    check_one_step(in);
    const mm::SlabPlan sp = mm::slab_plan(in);
    EXPECT(sp.rows_per_wave == 8);
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

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "table") == 0) {
        for (const Case& c : kCases) std::printf("\"%s\",\n", case_text(c).c_str());
        return 0;
    }
    check_table();
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
    if (!g_failed) std::printf("ok\n");
    return g_failed;
}
