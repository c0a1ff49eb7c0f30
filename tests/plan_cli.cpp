// plan_cli.cpp -- the host-only planner (mpi-model_amd/csrc/mm_plan.cpp) behind a line
// protocol, for tests/test_plan.py: commands on stdin, one line of integers per query on
// stdout. Built with plain g++ (no ROCm headers), also under -fsanitize=address,undefined.
//   env NAME VALUE | envclear        MM_* variables of the next `in`
//   in H W x_init h nranks n_attr split n_passes diffuse_mask chains ring ncu swpc
//        swpc: mm_info.seg_waves_per_cu of the device (waves; a wide workgroup's slots x
//        its waves), handed to the planner as the slots of every instance
//   plan n | kern k | info | graph nsteps reduce_every any | launch k red
//   cap k                            passk_max_rows(k, pitch), the same spelled out, the even cut
//   seg kernel k slots n0 n1 ns      segments() alone for n = n0..n1 rows: th th_edge count cap
#include <algorithm>
#include <cstdio>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "../mpi-model_amd/csrc/mm_plan.hpp"

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
            int split, chains, ring, swpc;
            in = mm::PlanIn();
            is >> in.H >> in.W >> in.x_init >> in.h >> in.nranks >> in.n_attr >> split >>
                in.n_passes >> in.diffuse_mask >> chains >> ring >> in.ncu >> swpc;
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
        } else if (cmd == "plan") {
            long long n;
            is >> n;
            for (int k : mm::pass_lengths(in, n)) std::printf("%d ", k);
            std::printf("\n");
        } else if (cmd == "kern") {
            int k;
            is >> k;
            const mm::KernelChoice c = mm::kernel_for(in, k);
            std::printf("%d %d %lld\n", (int)c.kernel, c.cols, c.strips);
        } else if (cmd == "info") {
            const mm::SlabPlan s = mm::slab_plan(in);
            std::printf("%d %d %d %lld %d\n", (int)s.kernel, s.steps_per_launch, s.rows_per_wave,
                        s.waves_per_pass, s.seg_waves_per_cu);
        } else if (cmd == "graph") {
            long long n, re;
            int any;
            is >> n >> re >> any;
            std::printf("%lld\n", mm::graph_per(in, n, re, any != 0));
        } else if (cmd == "seg") {
            int kernel, k, slots;
            long long n0, n1, ns;
            is >> kernel >> k >> slots >> n0 >> n1 >> ns;
            for (long long n = n0; n <= n1; ++n) {
                const mm::Segments s = mm::segments(in, (mm::Kernel)kernel, k, slots, n, ns);
                std::printf("%d %d %lld %lld\n", s.th, s.th_edge, s.count,
                            std::max<long long>(16, mm::passk_max_rows(k, in.pitch)));
            }
        } else if (cmd == "cap") {
            // the 2^31 offset cap of a k-step segment at this pitch, as the header states it
            // and spelled out, and the even length segments() cuts a capped segment to
            int k;
            is >> k;
            const long long cap = mm::passk_max_rows(k, in.pitch);
            std::printf("%lld %lld %lld\n", cap,
                        (1LL << 31) / (in.pitch * 8) - (3 * k + 2 * mm::kSegPrefetch1 + 8), cap & ~1LL);
        } else if (cmd == "launch") {
            int k, red;
            is >> k >> red;
            const mm::PassLaunches p = mm::pass_launches(in, k, red != 0);
            const mm::Launch &a = p.interior, &b = p.border;
            std::printf("%d %d %d  %lld %lld %d %d %lld %lld  %lld %lld %lld %lld %d %lld %lld  %lld %lld\n",
                        (int)p.kern.kernel, (int)p.split, p.depth, a.lo, a.hi, a.th, a.th_edge,
                        a.waves_total, a.partial_base, b.lo, b.hi, b.lo2, b.hi2, b.th,
                        b.waves_total, b.partial_base, p.total, mm::partials_need(in));
        } else {
            std::fprintf(stderr, "plan_cli: unknown command '%s'\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
