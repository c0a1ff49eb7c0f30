// plan_fieldk_chain_cli.cpp -- the host-only planner (mpi-model_amd/csrc/mm_plan.cpp) on
// K-step rate-field passes of slabs with a halo (MM_FIELD_HALO, mm::field_k_for, the split
// plan of mm_fieldk_kernel), for tests/test_fieldk_chain_cpu.py. Built with plain g++ (no
// ROCm headers). Prints one line per failed check and exits 1, else "ok <kFieldMaxSteps>".
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

// The launches of every pass length of a chain slab whose field_k is K.
void check_split(const mm::PlanIn& base, int K) {
    mm::PlanIn in = base;
    in.field_k = K;
    const long long h = in.h;
    EXPECT(mm::kstep_ok(in) && mm::steps_per_launch(in) == K);
    EXPECT(mm::slab_plan(in).kernel == mm::kFieldK && mm::slab_plan(in).steps_per_launch == K);
    for (int k = 2; k <= K; ++k)
        for (int red = 0; red < 2; ++red) {
            const mm::PassLaunches p = mm::pass_launches(in, k, red);
            const long long ns = ceil_div(in.W, mm::passk_out_cols(k));
            EXPECT(p.kern.kernel == mm::kFieldK && p.kern.cols == 2 && p.kern.strips == ns);
            EXPECT(p.depth == k);
            EXPECT(p.split == (h >= 2 * k + 1));
            const mm::Launch& a = p.interior;
            EXPECT(a.seg == 1 && a.nstrips == ns && a.xcd_remap == 0 && a.partial_base == 0);
            EXPECT(a.waves_a == a.waves_total);
            EXPECT(a.waves_total == mm::seg_wave_count(a.hi - a.lo, ns, a.th, a.th_edge));
            EXPECT(a.th >= 16 && a.th_edge >= 8);
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
            EXPECT(p.total * k <= mm::partials_need(in));
        }
    // a pass of one step stays on the one-step kernel, split into one-row borders
    const mm::PassLaunches one = mm::pass_launches(in, 1, false);
    EXPECT(one.kern.kernel == mm::kOneStep && one.depth == 1 && one.split == (h >= 3));
}

// Balanced lengths, never above min(field_k, min_rows).
void check_lengths(const mm::PlanIn& base, int K) {
    mm::PlanIn in = base;
    in.field_k = K;
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
    // MM_FIELD_HALO: 1..kFieldMaxSteps are kept; unset, 0, 5, -1 and garbage are 1
    EXPECT(mm::kFieldMaxSteps == 4);
    EXPECT(mm::Knobs().field_halo == 1);
    EXPECT(knobs_of("MM_FIELD_STEPS", "4").field_halo == 1);
    for (int d = 1; d <= mm::kFieldMaxSteps; ++d)
        EXPECT(knobs_of("MM_FIELD_HALO", std::to_string(d).c_str()).field_halo == d);
    for (const char* bad : {"0", "5", "-1", "garbage", "", "1000000000000", "4x"}) {
        const int want = std::strcmp(bad, "4x") == 0 ? 4 : 1;  // atoll's prefix, as every knob
        EXPECT(knobs_of("MM_FIELD_HALO", bad).field_halo == want);
    }
    EXPECT(knobs_of("MM_FIELD_HALO", "4").field_steps == 0);

    // field_k_for: min(field_steps_for, MM_FIELD_HALO, min_rows) with a halo, under 2 off;
    // without a halo MM_FIELD_HALO changes nothing
    const long long shapes[][3] = {{77, 300, 4}, {27, 257, 3}, {24, 257, 3}, {16, 130, 8}, {40, 130, 2}};
    for (const auto& s : shapes)
        for (int g = 0; g < (int)s[2]; ++g) {
            mm::PlanIn in = slab(s[0], s[1], (int)s[2], g);
            const long long hmin = s[0] / s[2];
            EXPECT(in.min_rows == hmin);
            EXPECT(mm::field_k_for(in, true) == 0);  // nothing set: small slab, one step
            for (int K = 1; K <= mm::kFieldMaxSteps; ++K) {
                in.knobs = mm::Knobs();
                in.knobs.th = 8;
                in.knobs.field_steps = K;
                EXPECT(mm::field_k_for(in, true) == 0);  // MM_FIELD_STEPS alone: today's chain
                for (int d = 1; d <= mm::kFieldMaxSteps; ++d) {
                    in.knobs.field_halo = d;
                    const long long k = std::min<long long>(std::min(K, d), hmin);
                    EXPECT(mm::field_k_for(in, true) == (k >= 2 ? k : 0));
                    EXPECT(mm::field_k_for(in, false) == (K >= 2 ? K : 0));
                }
                in.knobs.field_halo = 4;
                in.knobs.passk = false;  // MM_PASSK=0
                EXPECT(mm::field_k_for(in, true) == 0);
            }
        }
    // the auto rule in a chain: by the cells of the chain's thinnest slab, never below the
    // single slab's threshold, the same K on every rank
    {
        mm::PlanIn a = slab(4096, 2048, 2, 0), b = slab(4096, 2048, 2, 1);
        EXPECT(mm::field_k_for(a, true) == 0 && mm::field_k_for(b, true) == 0);
        a.knobs.field_halo = b.knobs.field_halo = 4;
        const int ka = mm::field_k_for(a, true);
        EXPECT(ka == mm::field_k_for(b, true) && (ka == 0 || ka == 4));
        mm::PlanIn big = slab(65536, 32768, 8, 3);
        big.knobs.field_halo = 3;
        EXPECT(mm::field_k_for(big, true) == 3);
        big.knobs.field_halo = 4;
        EXPECT(mm::field_k_for(big, true) == 4);
        // uneven slabs (4097 rows in 2: 2048 and 2049) plan alike
        mm::PlanIn u0 = slab(4097, 2048, 2, 0), u1 = slab(4097, 2048, 2, 1);
        u0.knobs.field_halo = u1.knobs.field_halo = 4;
        EXPECT(u0.h != u1.h && mm::field_k_for(u0, true) == mm::field_k_for(u1, true));
        mm::PlanIn small = slab(4094, 2048, 2, 0);  // 2047 rows: below 2^22 cells
        small.knobs.field_halo = 4;
        EXPECT(mm::field_k_for(small, true) == 0);
        small.knobs.field_steps = 4;  // forcing stays
        EXPECT(mm::field_k_for(small, true) == 4);
    }

    // the split plan on the shapes of the GPU test, every slab, requested K = 2..4
    for (const auto& s : shapes)
        for (int g = 0; g < (int)s[2]; ++g)
            for (int K = 2; K <= mm::kFieldMaxSteps; ++K) {
                mm::PlanIn in = slab(s[0], s[1], (int)s[2], g);
                in.knobs.field_steps = K;
                in.knobs.field_halo = 4;
                const int k = mm::field_k_for(in, true);
                EXPECT(k == (int)std::min<long long>(K, s[0] / s[2]));
                check_split(in, k);
                check_lengths(in, k);
            }
    {
        mm::PlanIn in = slab(27, 257, 3, 1);
        in.field_k = 4;
        EXPECT(mm::pass_lengths(in, 7) == (std::vector<int>{4, 3}));
        EXPECT(mm::pass_launches(in, 4, true).split);         // h = 9 = 2K + 1
        EXPECT(mm::pass_launches(in, 4, true).interior.hi - mm::pass_launches(in, 4, true).interior.lo == 1);
        in = slab(24, 257, 3, 1);
        in.field_k = 4;
        EXPECT(!mm::pass_launches(in, 4, true).split && mm::pass_launches(in, 3, true).split);
        in = slab(16, 130, 8, 5);
        in.knobs.field_steps = in.knobs.field_halo = 4;
        EXPECT(mm::field_k_for(in, true) == 2);
        in.field_k = 2;
        EXPECT(mm::pass_lengths(in, 7) == (std::vector<int>{2, 2, 2, 1}));
        EXPECT(!mm::pass_launches(in, 2, false).split);
    }
    // at size: the slab of the GPU test and a production slab, split, with and without sums
    for (int K = 2; K <= mm::kFieldMaxSteps; ++K) {
        check_split(slab(4096, 2048, 2, 1), K);
        check_split(slab(32768, 32768, 8, 3), K);
        mm::PlanIn self = slab(8192, 8192, 1, 0);  // MM_SELF_HALO: one rank, split
        self.split = true;
        check_split(self, K);
    }

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
        const size_t knob = text.find("MM_FIELD_HALO", env);
        EXPECT(knob != std::string::npos && knob < create);
        const size_t lock = text.find("runs in lockstep");
        EXPECT(lock != std::string::npos && text.find("MM_FIELD_HALO", lock) < create);
        const size_t up0 = text.find("/* The rate field of attribute attr");
        const size_t up1 = text.find("int mm_rate_field_upload(");
        EXPECT(up0 != std::string::npos && up1 != std::string::npos && up0 < up1);
        const std::string up = text.substr(up0, up1 - up0);
        EXPECT(up.find("MM_FIELD_HALO") != std::string::npos);
        EXPECT(up.find("MM_ERR_STATE") != std::string::npos && up.find("halo_depth") != std::string::npos);
        EXPECT(text.find("#define MM_ABI_VERSION 3") != std::string::npos);
    }

    if (!g_failed) std::printf("ok %d\n", mm::kFieldMaxSteps);
    return g_failed;
}
