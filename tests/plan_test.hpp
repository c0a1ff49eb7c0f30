// plan_test.hpp -- what the checking programs of the host-only units share (plan_field_cli,
// plan_fieldk_cli, plan_fieldk_chain_cli, plan_closed_cli, plan_closedk_cli, program_cli):
// EXPECT, a slab's mm::PlanIn as the engine fills it, knobs from a stand-in environment, flow
// lists, and a plan as text. Built with plain g++ (no ROCm headers).
#pragma once

#include <algorithm>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "../include/mpimodel.h"
#include "../mpi-model_amd/csrc/mm_program.hpp"

namespace {

int g_failed = 0;

// Prints one line per failed check; main returns g_failed.
void expect(bool ok, const char* what, int line) {
    if (ok) return;
    std::printf("line %d: %s\n", line, what);
    g_failed = 1;
}
#define EXPECT(c) expect((c), #c, __LINE__)

[[maybe_unused]] long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }

// Slab g of G of an H x W grid (mm_partition_rows), as the engine fills mm::PlanIn.
[[maybe_unused]] mm::PlanIn slab(long long H, long long W, int G, int g, int n_attr, bool split) {
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

[[maybe_unused]] mm::Knobs knobs_of(const std::map<std::string, std::string>& env) {
    return mm::read_knobs([&](const char* name) -> const char* {
        const auto it = env.find(name);
        return it == env.end() ? nullptr : it->second.c_str();
    });
}

[[maybe_unused]] mm::Knobs knobs_of(const char* name, const char* value) {
    return knobs_of({{name, value}});
}

// Flows as mm_add_flow stores them.
[[maybe_unused]] mm::Flow D(int a, double rate = 0.1) { return {MM_FLOW_DIFFUSE, a, a, rate}; }
[[maybe_unused]] mm::Flow T(int a, int b, double rate = 0.05) { return {MM_FLOW_TRANSFER, a, b, rate}; }
[[maybe_unused]] mm::Flow F(int a) { return {MM_FLOW_DIFFUSE_FIELD, a, a, 0.0}; }
[[maybe_unused]] mm::Flow C(int a) { return {MM_FLOW_DIFFUSE_CLOSED, a, a, 0.0}; }

// `in` with the program of `flows`, as the engine describes it after the last mm_add_flow.
[[maybe_unused]] mm::PlanIn with_flows(mm::PlanIn in, const std::vector<mm::Flow>& flows, bool halo) {
    mm::set_program(in, mm::compile_passes(flows), halo, in.knobs.th);
    return in;
}

[[maybe_unused]] std::string launch_text(const mm::Launch& l) {
    char buf[256];
    std::snprintf(buf, sizeof buf, "%lld-%lld,%lld-%lld s%d th%d/%d x%d n%d w%lld/%lld b%lld", l.lo, l.hi,
                  l.lo2, l.hi2, l.seg, l.th, l.th_edge, l.xcd_remap, l.nstrips, l.waves_a,
                  l.waves_total, l.partial_base);
    return buf;
}

// Everything the engine asks the planner about a program, as one line.
[[maybe_unused]] std::string plan_text(const mm::PlanIn& in) {
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

// A program with a rate-field pass whose field_k (and closed_k) is 0: one step per pass on the
// one-step schedule, whatever the rest of the input says.
[[maybe_unused]] void check_one_step(const mm::PlanIn& on) {
    EXPECT(on.field && on.field_k == 0);
    EXPECT(!mm::passk_ok(on) && !mm::kstep_ok(on));
    EXPECT(mm::steps_per_launch(on) == 1);
    EXPECT(mm::pass_lengths(on, 7) == std::vector<int>(7, 1));
    EXPECT(mm::next_pass_len(on, 20) == 1);
    EXPECT(mm::kernel_for(on, 1).kernel == mm::kOneStep);
    EXPECT(mm::kernel_for(on, 4).kernel == mm::kOneStep);
    EXPECT(mm::slab_plan(on).kernel == mm::kOneStep);
    EXPECT(mm::slab_plan(on).steps_per_launch == 1);
    for (int red = 0; red < 2; ++red) {
        const mm::PassLaunches p = mm::pass_launches(on, 1, red != 0);
        EXPECT(p.kern.kernel == mm::kOneStep);
        EXPECT(p.depth == 1);
        const long long h = on.h, ns = on.pitch / mm::kStripCols;
        EXPECT(p.interior.nstrips == ns);
        EXPECT(p.interior.th == 8 && p.interior.seg == 0);
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

}  // namespace
