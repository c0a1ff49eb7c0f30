// plan_closedk_chain_cli.cpp -- the host-only planner (mpi-model_amd/csrc/mm_plan.cpp) on
// K-step closed rate-field passes of slabs with a halo (MM_CLOSED_HALO, mm::closed_k_for, the
// split plan of mm_closedk_kernel), for tests/test_closedk_chain_cpu.py. Built with plain g++
// (no ROCm headers).
//   * MM_CLOSED_HALO keeps 2..kClosedMaxSteps + 1; anything else is unset (0).
//   * With a halo closed_k_for = min(MM_CLOSED_STEPS, MM_CLOSED_HALO - 1, min_rows), off under
//     2; MM_FIELD_HALO changes no plan of a closed program (tests/program_cli.cpp pins that a
//     closed program under MM_FIELD_HALO=4 on a slab with a halo stays at one step per pass),
//     and without a halo neither knob changes anything.
//   * The split plan: depth K, split from h = 2K + 1 rows on, interior segments of rows
//     [K, h-K), border blocks of kBorderRows rows behind the interior's partials, over
//     ceil(W / closedk_out_cols(k)) strips; a thinner slab one segment launch.
//   * Every slab of a chain plans the same K and the same pass lengths.
//   * With MM_CLOSED_HALO unset every line of tests/plan_closed_table.inc is reproduced.
// Prints one line per failed check and exits 1, else "ok <kClosedMaxSteps>".
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "plan_closed_cases.hpp"

namespace {

using Env = std::map<std::string, std::string>;

// Slab g of G of an H x W grid, one attribute, a halo (a chain, or G == 1 with a halo mode), the
// program one closed diffusion, 8 slots per CU whatever the kernel.
mm::PlanIn chain_slab(long long H, long long W, int G, int g, const Env& env) {
    mm::PlanIn in = slab(H, W, G, g, 1, true);
    in.knobs = knobs_of(env);
    in.slots = [](mm::Kernel, int, bool) { return 8; };
    in = with_flows(in, {C(0)}, true);
    EXPECT(in.closed && in.field && in.n_passes == 1 && in.field_k == 0 && in.knobs.th == 8);
    return in;
}

Env env_of(int steps, int field_halo, int closed_halo) {
    Env e;
    if (steps >= 0) e["MM_CLOSED_STEPS"] = std::to_string(steps);
    if (field_halo >= 0) e["MM_FIELD_HALO"] = std::to_string(field_halo);
    if (closed_halo >= 0) e["MM_CLOSED_HALO"] = std::to_string(closed_halo);
    return e;
}

// The launches of every pass length of a slab with a halo whose closed_k is K.
void check_split(const mm::PlanIn& in, int K) {
    const long long h = in.h;
    EXPECT(in.closed_k == K && mm::kstep_ok(in) && !mm::passk_ok(in));
    EXPECT(mm::steps_per_launch(in) == K);
    EXPECT(mm::slab_plan(in).kernel == mm::kClosedK && mm::slab_plan(in).steps_per_launch == K);
    for (int k = 2; k <= K; ++k)
        for (int red = 0; red < 2; ++red) {
            const mm::PassLaunches p = mm::pass_launches(in, k, red);
            const long long ns = ceil_div(in.W, mm::closedk_out_cols(k));
            EXPECT(p.kern.kernel == mm::kClosedK && (int)p.kern.kernel == 5 && p.kern.cols == 2);
            EXPECT(p.kern.strips == ns);
            EXPECT(p.depth == k);
            EXPECT(p.split == (h >= 2 * k + 1));
            const mm::Launch& a = p.interior;
            EXPECT(a.seg == 1 && a.nstrips == ns && a.xcd_remap == 0 && a.partial_base == 0);
            EXPECT(a.waves_a == a.waves_total);
            EXPECT(a.waves_total == mm::seg_wave_count(a.hi - a.lo, ns, a.th, a.th_edge));
            EXPECT(a.th >= 16 && a.th == a.th_edge);
            if (p.split) {
                EXPECT(a.lo == k && a.hi == h - k && a.waves_total >= ns);
                const mm::Launch& b = p.border;
                EXPECT(b.seg == 0 && b.th == mm::kBorderRows && b.nstrips == ns);
                EXPECT(b.lo == 0 && b.hi == k && b.lo2 == h - k && b.hi2 == h);
                // K <= kBorderRows rows a side: one block per strip and side
                EXPECT(b.waves_a == ns && b.waves_total == 2 * ns);
                EXPECT(b.partial_base == a.waves_total);
                EXPECT(p.total == a.waves_total + b.waves_total);
            } else {  // too thin: one segment launch over the whole slab after the exchange
                EXPECT(a.lo == 0 && a.hi == h && p.border.waves_total == 0);
                EXPECT(p.total == a.waves_total);
            }
            EXPECT(p.total * mm::kClosedMaxSteps <= mm::partials_need(in));
        }
    // a pass of one step stays on the one-step kernel, split into one-row borders
    const mm::PassLaunches one = mm::pass_launches(in, 1, false);
    EXPECT(one.kern.kernel == mm::kOneStep && one.depth == 1 && one.split == (h >= 3));
    // a graph holds whole passes and an even number of flips
    EXPECT(mm::graph_per(in, 64 * K, 0) % (2 * K) == 0);
}

// Balanced lengths, never above min(closed_k, min_rows).
void check_lengths(const mm::PlanIn& in, int K) {
    for (long long n : {1LL, 2LL, 5LL, 7LL, 20LL, 64LL, 1000LL}) {
        const std::vector<int> lens = mm::pass_lengths(in, n);
        long long sum = 0;
        int lo = K, hi = 0;
        for (int l : lens) {
            sum += l;
            lo = std::min(lo, l), hi = std::max(hi, l);
        }
        EXPECT(sum == n && hi <= K && hi <= in.min_rows && lo >= 1 && hi - lo <= 1);
        EXPECT((long long)lens.size() == ceil_div(n, K));
    }
}

}  // namespace

int main(int argc, char** argv) {
    EXPECT(mm::kClosedMaxSteps == 4 && mm::kBorderRows == 4);
    // MM_CLOSED_HALO: 2..kClosedMaxSteps + 1 are kept; unset, 0, 1, 6, x and the rest are unset
    EXPECT(mm::Knobs().closed_halo == 0 && knobs_of({}).closed_halo == 0);
    for (int d = 2; d <= mm::kClosedMaxSteps + 1; ++d) {
        const mm::Knobs k = knobs_of("MM_CLOSED_HALO", std::to_string(d).c_str());
        EXPECT(k.closed_halo == d && k.field_halo == 1 && k.closed_steps == 0 && k.field_steps == 0);
        EXPECT(mm::closed_field_promise(k) == d);
    }
    for (const char* bad : {"1", "6", "x", "0", "-2", "", "1000000000000", "99"})
        EXPECT(knobs_of("MM_CLOSED_HALO", bad).closed_halo == 0);
    EXPECT(knobs_of("MM_CLOSED_HALO", "5x").closed_halo == 5);  // atoll's prefix, as every knob
    EXPECT(knobs_of("MM_FIELD_HALO", "4").closed_halo == 0);
    EXPECT(knobs_of("MM_FIELD_HALO", "5").field_halo == 1);  // MM_FIELD_HALO still stops at 4
    EXPECT(mm::closed_field_promise(knobs_of(env_of(-1, 4, 2))) == 4);
    EXPECT(mm::closed_field_promise(knobs_of(env_of(-1, 2, 5))) == 5);
    EXPECT(mm::closed_field_promise(knobs_of({})) == 1);

    // closed_k_for over (MM_CLOSED_STEPS, MM_FIELD_HALO, MM_CLOSED_HALO, min_rows), every slab
    const long long shapes[][3] = {{77, 300, 4}, {27, 257, 3}, {24, 257, 3}, {16, 130, 8}, {40, 130, 2}};
    for (const auto& s : shapes)
        for (int g = 0; g < (int)s[2]; ++g) {
            const long long hmin = s[0] / s[2];
            for (int K = -1; K <= mm::kClosedMaxSteps + 1; ++K)
                for (int fh = -1; fh <= 4; ++fh)
                    for (int ch = -1; ch <= mm::kClosedMaxSteps + 2; ++ch) {
                        const mm::PlanIn in = chain_slab(s[0], s[1], (int)s[2], g, env_of(K, fh, ch));
                        EXPECT(in.min_rows == hmin);
                        const int steps = std::min(std::max(K, 0), mm::kClosedMaxSteps);
                        const int promise = ch >= 2 && ch <= 5 ? ch : 0;  // whatever MM_FIELD_HALO is
                        const long long k = std::min<long long>(std::min(steps, promise - 1), hmin);
                        EXPECT(mm::closed_field_promise(in.knobs) == std::max(fh >= 1 ? fh : 1, promise));
                        EXPECT(in.closed_k == (k >= 2 ? (int)k : 0));
                        EXPECT(mm::closed_k_for(in, true) == in.closed_k);
                        // without a halo the promise and the chain do not matter
                        EXPECT(mm::closed_k_for(in, false) == (steps >= 2 ? steps : 0));
                        mm::PlanIn off = in;
                        off.knobs.passk = false;  // MM_PASSK=0
                        EXPECT(mm::closed_k_for(off, true) == 0);
                        if (in.closed_k == 0) check_one_step(in);
                    }
        }
    {
        // MM_FIELD_HALO alone fuses nothing; MM_CLOSED_HALO=d reaches d - 1, 5 reaches 4;
        // MM_CLOSED_HALO=2 alone is the one-step pass's promise
        EXPECT(chain_slab(77, 300, 4, 1, env_of(4, 4, -1)).closed_k == 0);
        EXPECT(chain_slab(77, 300, 4, 1, env_of(4, 3, -1)).closed_k == 0);
        EXPECT(chain_slab(77, 300, 4, 1, env_of(4, 2, -1)).closed_k == 0);
        EXPECT(chain_slab(77, 300, 4, 1, env_of(4, 4, 4)).closed_k == 3);
        EXPECT(chain_slab(77, 300, 4, 1, env_of(4, -1, 3)).closed_k == 2);
        EXPECT(chain_slab(77, 300, 4, 1, env_of(4, -1, 5)).closed_k == 4);
        EXPECT(chain_slab(77, 300, 4, 1, env_of(4, 4, 5)).closed_k == 4);
        EXPECT(chain_slab(77, 300, 4, 1, env_of(4, -1, 2)).closed_k == 0);
        EXPECT(chain_slab(77, 300, 4, 1, env_of(2, -1, 5)).closed_k == 2);
        EXPECT(chain_slab(77, 300, 4, 1, env_of(-1, -1, 5)).closed_k == 0);  // no auto rule
        EXPECT(chain_slab(77, 300, 4, 1, env_of(1, -1, 5)).closed_k == 0);
        // the engine's conditions, through real flow lists
        const mm::PlanIn on = chain_slab(77, 300, 4, 1, env_of(4, -1, 5));
        EXPECT(with_flows(on, {C(0), C(0)}, true).closed_k == 0);
        EXPECT(with_flows(on, {T(0, -1), C(0)}, true).closed_k == 0);
        EXPECT(with_flows(on, {F(0)}, true).closed_k == 0);
        mm::PlanIn two = on;
        two.n_attr = 2;
        EXPECT(with_flows(two, {C(0)}, true).closed_k == 0);
        // a pitch whose closedk_max_rows is under 64
        mm::PlanIn wide = on;
        wide.pitch = 1LL << 22;
        EXPECT(mm::closed_k_for(wide, true) == 0);
    }

    // the split plan on the shapes of the GPU test, every slab, requested K = 2..4
    for (const auto& s : shapes)
        for (int K = 2; K <= mm::kClosedMaxSteps; ++K) {
            std::string first;
            for (int g = 0; g < (int)s[2]; ++g) {
                const mm::PlanIn in = chain_slab(s[0], s[1], (int)s[2], g, env_of(K, -1, K + 1));
                const int k = (int)std::min<long long>(K, s[0] / s[2]);
                check_split(in, k);
                check_lengths(in, k);
                // rank-invariance: K and the pass lengths of every run
                std::string text = std::to_string(in.closed_k) + ":";
                for (long long n : {1LL, 5LL, 7LL, 20LL})
                    for (int l : mm::pass_lengths(in, n)) text += std::to_string(l) + ",";
                if (g == 0) first = text;
                EXPECT(text == first);
            }
        }
    {
        mm::PlanIn in = chain_slab(27, 257, 3, 1, env_of(4, -1, 5));
        EXPECT(in.closed_k == 4 && in.h == 9);
        EXPECT(mm::pass_lengths(in, 7) == (std::vector<int>{4, 3}));
        const mm::PassLaunches p = mm::pass_launches(in, 4, true);
        EXPECT(p.split && p.interior.lo == 4 && p.interior.hi == 5);  // h = 9 = 2K + 1
        EXPECT(p.kern.strips == ceil_div(257, mm::closedk_out_cols(4)) && p.kern.strips == 3);
        EXPECT(p.border.partial_base == p.interior.waves_total && p.border.waves_total == 6);
        in = chain_slab(24, 257, 3, 1, env_of(4, -1, 5));
        EXPECT(in.h == 8 && !mm::pass_launches(in, 4, true).split && mm::pass_launches(in, 3, true).split);
        in = chain_slab(16, 130, 8, 5, env_of(4, -1, 5));
        EXPECT(in.h == 2 && in.closed_k == 2);  // capped by min_rows
        EXPECT(mm::pass_lengths(in, 7) == (std::vector<int>{2, 2, 2, 1}));
        EXPECT(!mm::pass_launches(in, 2, false).split);
        // uneven slabs plan alike
        const mm::PlanIn u0 = chain_slab(4097, 2048, 2, 0, env_of(4, -1, 5));
        const mm::PlanIn u1 = chain_slab(4097, 2048, 2, 1, env_of(4, -1, 5));
        EXPECT(u0.h != u1.h && u0.closed_k == 4 && u1.closed_k == 4);
    }
    // at size: a production slab and the self-halo slabs (one rank, split), with and without sums
    for (int K = 2; K <= mm::kClosedMaxSteps; ++K) {
        check_split(chain_slab(32768, 32768, 8, 3, env_of(K, -1, K + 1)), K);
        check_split(chain_slab(2048, 2048, 1, 0, env_of(K, -1, K + 1)), K);
        check_split(chain_slab(8192, 8192, 1, 0, env_of(K, -1, 5)), K);
    }
    EXPECT(mm::pass_launches(chain_slab(2048, 2048, 1, 0, env_of(4, -1, 5)), 4, true).kern.strips == 18);

    // MM_CLOSED_HALO unset: the recorded plans, line for line, whatever MM_CLOSED_STEPS says
    check_table();
    check_table(mm::kClosedMaxSteps);

    // header text: argv[1] = include/mpimodel.h
    if (argc > 1) {
        std::string text;
        if (FILE* f = std::fopen(argv[1], "rb")) {
            char buf[4096];
            for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, n);
            std::fclose(f);
        }
        const size_t env = text.find("Environment:"), create = text.find("int mm_engine_create(");
        EXPECT(env != std::string::npos && create != std::string::npos && env < create);
        const size_t knob = text.find("MM_CLOSED_HALO", env);
        EXPECT(knob != std::string::npos && knob < create);
        const size_t lock = text.find("runs in lockstep");
        EXPECT(lock != std::string::npos && text.find("MM_CLOSED_HALO", lock) < create);
        EXPECT(text.find("#define MM_ABI_VERSION 3") != std::string::npos);
    }

    if (!g_failed) std::printf("ok %d\n", mm::kClosedMaxSteps);
    return g_failed;
}
