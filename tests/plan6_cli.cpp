// plan6_cli.cpp -- the host-only planner (mpi-model_amd/csrc/mm_plan.cpp) behind a line
// protocol for tests/test_plan_wide6.py: tests/plan_cli.cpp's protocol with the fused
// six-column instance's occupancy as one more plan input. Plain g++, no ROCm headers.
//   env NAME VALUE | envclear        MM_* variables of the next `in`
//   in H W x_init h nranks n_attr split n_passes diffuse_mask chains ring ncu swpc s6
//        s6: workgroup slots per CU of the fused instance; 0: the planner is given none
//   kern k red | info | plan n
//   launch k red                     the pass's launches, every field (both launches' Wide6 too)
#include <algorithm>
#include <cstdio>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "../mpi-model_amd/csrc/mm_plan.hpp"

static void print_launch(const mm::Launch& l) {
    const mm::Wide6& w = l.c6;
    std::printf(" %lld %lld %lld %lld %d %d %d %d %d %lld %lld %lld  %d %d %d %d %d %d %d %lld %lld %lld ",
                l.lo, l.hi, l.lo2, l.hi2, l.seg, l.th, l.th_edge, l.xcd_remap, l.nstrips, l.waves_a,
                l.waves_total, l.partial_base, w.top, w.bot, w.col, w.rcol, w.strips, w.rstrips,
                w.th, w.band0, w.band1, w.frame);
}

int main() {
    std::map<std::string, std::string> env;
    mm::PlanIn in;
    std::string line, cmd;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        if (!(is >> cmd)) continue;
        if (cmd == "env") {
            std::string name, value;
            is >> name >> value;
            env[name] = value;
        } else if (cmd == "envclear") {
            env.clear();
        } else if (cmd == "in") {
            int split, chains, ring, swpc, s6;
            in = mm::PlanIn();
            is >> in.H >> in.W >> in.x_init >> in.h >> in.nranks >> in.n_attr >> split >>
                in.n_passes >> in.diffuse_mask >> chains >> ring >> in.ncu >> swpc >> s6;
            in.split = split, in.chains = chains;
            in.knobs = mm::read_knobs([&](const char* n) {
                auto it = env.find(n);
                return it == env.end() ? nullptr : it->second.c_str();
            });
            in.ring = ring && in.knobs.ring_ok;
            in.pitch = (in.W + mm::kStripCols - 1) / mm::kStripCols * mm::kStripCols;
            in.min_rows = std::min(in.h, in.H / in.nranks);
            const mm::PlanIn* p = &in;
            in.slots = [p, swpc](mm::Kernel kernel, int k, bool) {
                if (kernel != mm::kWide) return swpc;
                const int c = p->n_attr > 1 ? 2 : 4;
                return swpc / std::max(1, mm::wide_waves_per_block(k, c, p->n_attr, p->ring));
            };
            if (s6 > 0) in.slots6 = [s6](int) { return s6; };
        } else if (cmd == "plan") {
            long long n;
            is >> n;
            for (int k : mm::pass_lengths(in, n)) std::printf("%d ", k);
            std::printf("\n");
        } else if (cmd == "kern") {
            int k, red;
            is >> k >> red;
            const mm::KernelChoice c = mm::kernel_for(in, k, red != 0);
            std::printf("%d %d %lld\n", (int)c.kernel, c.cols, c.strips);
        } else if (cmd == "info") {
            const mm::SlabPlan s = mm::slab_plan(in);
            std::printf("%d %d %d %lld %d\n", (int)s.kernel, s.steps_per_launch, s.rows_per_wave,
                        s.waves_per_pass, s.seg_waves_per_cu);
        } else if (cmd == "launch") {
            int k, red;
            is >> k >> red;
            const mm::PassLaunches p = mm::pass_launches(in, k, red != 0);
            std::printf("%d %d %lld %d %d %lld ", (int)p.kern.kernel, p.kern.cols, p.kern.strips,
                        p.depth, (int)p.split, p.total);
            print_launch(p.interior);
            print_launch(p.border);
            std::printf("%lld\n", mm::partials_need(in));
        } else {
            std::fprintf(stderr, "plan6_cli: unknown command '%s'\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
