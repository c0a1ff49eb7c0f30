// program_cli.cpp -- the host-only unit that turns a flow list into the planner's input
// (mpi-model_amd/csrc/mm_program.cpp: compile_passes, ring_program, set_program), for
// tests/test_program_cpu.py and tests/test_gpu_program.py. Built with plain g++ (no ROCm
// headers).
//   program_cli                  checks the unit; prints one line per failed check and exits 1,
//                                else "ok"
//   program_cli print H W n_attr FLOW... [NAME=VALUE...]
//                                what an engine of one H x W slab without a halo reports for the
//                                program under that environment, as one line of integers:
//                                n_passes, kernel, steps_per_launch | the pass lengths of 7 steps
//                                | kernel, columns per lane, strips of a pass of each kPrintK
//                                steps. FLOW: D<a> F<a> C<a> T<a><b>.
// The expected passes of kPassCases were recorded from the engine's own compile_passes before
// it moved here; the notation is {pre, diffuse_mask, post, field_mask, closed}.
#include <cstdlib>
#include <cstring>

#include "plan_test.hpp"

namespace {

using Flows = std::vector<mm::Flow>;

const int kPrintK[] = {1, 2, 3, 4, 8, 20};

std::string passes_text(const std::vector<mm::Pass>& passes) {
    std::string s;
    char buf[96];
    for (const mm::Pass& p : passes) {
        std::snprintf(buf, sizeof buf, "%s{%d,%d,%d,%d,%d}", s.empty() ? "" : " ", (int)p.pre.size(),
                      p.diffuse_mask, (int)p.post.size(), p.field_mask, (int)p.closed);
        s += buf;
    }
    return s;
}

const Flows kC5 = {T(0, 1), T(1, 2), T(2, 3), T(3, 0), D(0), D(1), D(2), D(3)};
const Flows kFiveTransfers = {T(0, 1), T(1, 2), T(2, 3), T(3, 0), T(0, 1)};

struct PassCase {
    Flows flows;
    const char* passes;
};

const PassCase kPassCases[] = {
    {{D(0)}, "{0,1,0,0,0}"},
    {{D(0), D(0)}, "{0,1,0,0,0} {0,1,0,0,0}"},
    {{D(0), D(1)}, "{0,3,0,0,0}"},
    {{T(0, 1), D(0), T(1, 0)}, "{1,1,1,0,0}"},
    {{T(0, 1), D(0), T(1, 0), D(1)}, "{1,1,1,0,0} {0,2,0,0,0}"},
    {kFiveTransfers, "{4,0,0,0,0} {1,0,0,0,0}"},
    {{D(0), T(0, 1), T(1, 2), T(2, 3), T(3, 0), T(0, 1)}, "{0,1,4,0,0} {1,0,0,0,0}"},
    {{F(0), F(1)}, "{0,0,0,3,0}"},
    {{F(0), F(0)}, "{0,0,0,1,0} {0,0,0,1,0}"},
    {{F(0), D(0)}, "{0,0,0,1,0} {0,1,0,0,0}"},
    {{D(0), F(0)}, "{0,1,0,0,0} {0,0,0,1,0}"},
    {{T(0, 1), F(0)}, "{1,0,0,0,0} {0,0,0,1,0}"},
    {{C(0)}, "{0,0,0,1,1}"},
    {{F(1), C(0), F(1)}, "{0,0,0,2,0} {0,0,0,1,1} {0,0,0,2,0}"},
    {{C(0), C(0)}, "{0,0,0,1,1} {0,0,0,1,1}"},
    {{D(0), C(0), D(0)}, "{0,1,0,0,0} {0,0,0,1,1} {0,1,0,0,0}"},
    {kC5, "{4,15,0,0,0}"},
    {{}, ""},
};

void check_passes() {
    for (const PassCase& c : kPassCases) {
        const std::string got = passes_text(mm::compile_passes(c.flows));
        if (got != c.passes) {
            std::printf("passes changed:\n  was %s\n  is  %s\n", c.passes, got.c_str());
            g_failed = 1;
        }
    }
    // rates and operands land where their flows stood, in order
    const std::vector<mm::Pass> p =
        mm::compile_passes({T(0, 1, 0.25), T(2, -1, 0.5), D(0, 0.125), D(2, 0.375), T(1, 0, 0.75), D(1, 0.0625)});
    EXPECT(passes_text(p) == "{2,5,1,0,0} {0,2,0,0,0}");
    if (p.size() == 2 && p[0].pre.size() == 2 && p[0].post.size() == 1) {
        EXPECT(p[0].pre[0].a == 0 && p[0].pre[0].b == 1 && p[0].pre[0].rate == 0.25);
        EXPECT(p[0].pre[1].a == 2 && p[0].pre[1].b == -1 && p[0].pre[1].rate == 0.5);
        EXPECT(p[0].post[0].a == 1 && p[0].post[0].b == 0 && p[0].post[0].rate == 0.75);
        EXPECT(p[0].drate[0] == 0.125 && p[0].drate[1] == 0.0 && p[0].drate[2] == 0.375 && p[0].drate[3] == 0.0);
        EXPECT(p[1].drate[1] == 0.0625 && p[1].drate[0] == 0.0 && p[1].drate[2] == 0.0);
    }
    // the chain that overflows keeps its order across the passes
    const std::vector<mm::Pass> q = mm::compile_passes(
        {T(0, 1, 1.0), T(1, 2, 2.0), T(2, 3, 3.0), T(3, 0, 4.0), T(0, 2, 5.0)});
    if (q.size() == 2 && q[0].pre.size() == 4 && q[1].pre.size() == 1) {
        for (int t = 0; t < 4; ++t) EXPECT(q[0].pre[t].a == t && q[0].pre[t].rate == t + 1.0);
        EXPECT(q[1].pre[0].a == 0 && q[1].pre[0].b == 2 && q[1].pre[0].rate == 5.0);
    } else {
        EXPECT(!"five transfers: a chain of four and a pass of one");
    }
}

void check_ring() {
    const mm::Knobs on{}, off = knobs_of("MM_CHAIN_RING", "0");
    EXPECT(mm::ring_program(on, 4, mm::compile_passes(kC5)));
    EXPECT(!mm::ring_program(off, 4, mm::compile_passes(kC5)));
    Flows f = kC5;
    std::swap(f[1], f[2]);  // two transfers swapped
    EXPECT(!mm::ring_program(on, 4, mm::compile_passes(f)));
    f = kC5;
    f.pop_back();  // only three diffusions
    EXPECT(!mm::ring_program(on, 4, mm::compile_passes(f)));
    f = kC5;
    f.push_back(T(0, 1));  // a post-chain
    EXPECT(mm::compile_passes(f).size() == 1 && !mm::ring_program(on, 4, mm::compile_passes(f)));
    EXPECT(!mm::ring_program(on, 3, mm::compile_passes(kC5)));  // a three-attribute engine
    EXPECT(!mm::ring_program(on, 4, {}));
    // set_program stores it
    EXPECT(with_flows(slab(130, 97, 1, 0, 4, false), kC5, false).ring);
    mm::PlanIn no = slab(130, 97, 1, 0, 4, false);
    no.knobs = off;
    EXPECT(!with_flows(no, kC5, false).ring);
}

// `in` under `flows` on an engine created with MM_ROWS_PER_WAVE = th_env.
mm::PlanIn programmed(mm::PlanIn in, const Flows& flows, bool halo, int th_env) {
    mm::set_program(in, mm::compile_passes(flows), halo, th_env);
    return in;
}

void check_shape_and_rows() {
    mm::PlanIn one = slab(130, 97, 1, 0, 1, false), two = slab(130, 97, 1, 0, 2, false);
    // the shape of a one-pass program, and of others
    const mm::PlanIn d = programmed(one, {D(0)}, false, 32);
    EXPECT(d.n_passes == 1 && d.diffuse_mask == 1 && !d.chains && !d.ring && !d.field && !d.closed);
    const mm::PlanIn t = programmed(two, {T(0, 1), D(0), T(1, 0)}, false, 32);
    EXPECT(t.n_passes == 1 && t.diffuse_mask == 1 && t.chains && !t.field);
    const mm::PlanIn m = programmed(two, {D(0), D(0)}, false, 32);
    EXPECT(m.n_passes == 2 && m.diffuse_mask == 0 && !m.chains);
    const mm::PlanIn fc = programmed(two, {F(1), C(0), F(1)}, false, 32);
    EXPECT(fc.n_passes == 3 && fc.field && fc.closed);
    const mm::PlanIn f = programmed(one, {D(0), F(0)}, false, 32);
    EXPECT(f.n_passes == 2 && f.field && !f.closed);
    // knobs.th: the environment's height for one uniform diffusion of one attribute alone
    EXPECT(d.knobs.th == 32 && programmed(one, {D(0), D(0)}, false, 32).knobs.th == 32);
    EXPECT(programmed(one, {D(0)}, false, 16).knobs.th == 16);
    EXPECT(programmed(one, {T(0, -1), D(0)}, false, 32).knobs.th == 8);
    EXPECT(programmed(one, {D(0), T(0, -1)}, false, 32).knobs.th == 8);
    EXPECT(programmed(one, {F(0)}, false, 32).knobs.th == 8);
    EXPECT(programmed(one, {D(0), C(0)}, false, 32).knobs.th == 8);
    EXPECT(programmed(two, {D(0)}, false, 32).knobs.th == 8 && t.knobs.th == 8);
    // clearing gives the height back, to a reprogrammed PlanIn as to a fresh one
    mm::PlanIn re = programmed(one, {F(0)}, false, 32);
    mm::set_program(re, {}, false, 32);
    EXPECT(re.knobs.th == 32 && re.n_passes == 0 && !re.field && re.field_k == 0);
    mm::set_program(re, mm::compile_passes({D(0)}), false, 32);
    EXPECT(re.knobs.th == 32 && plan_text(re) == plan_text(d));
}

void check_field_k() {
    const long long shapes[][2] = {{130, 257}, {2048, 2048}, {8192, 8192}};
    for (int halo = 0; halo < 2; ++halo)
        for (int steps : {0, 1, 3, 4})
            for (int fh : {1, 4})
                for (const auto& s : shapes) {
                    mm::PlanIn in = slab(s[0], s[1], 1, 0, 1, halo != 0);
                    in.knobs.field_steps = steps, in.knobs.field_halo = fh;
                    const mm::PlanIn alone = with_flows(in, {F(0)}, halo != 0);
                    EXPECT(alone.field_k == mm::field_k_for(alone, halo != 0) && alone.closed_k == 0);
                    const int want = halo ? std::min(steps ? steps : (s[0] >= 2048 ? 4 : 0), fh)
                                          : (steps ? steps : (s[0] >= 2048 ? 4 : 0));
                    EXPECT(alone.field_k == (want >= 2 ? want : 0));
                    // any other program, or a second attribute: one step per pass
                    for (const Flows& f : {Flows{F(0), F(0)}, Flows{F(0), D(0)}, Flows{D(0), F(0)},
                                           Flows{T(0, -1), F(0)}, Flows{F(0), T(0, -1)}, Flows{C(0)},
                                           Flows{D(0)}, Flows{}})
                        EXPECT(with_flows(in, f, halo != 0).field_k == 0);
                    mm::PlanIn two = in;
                    two.n_attr = 2;
                    EXPECT(with_flows(two, {F(0)}, halo != 0).field_k == 0);
                    EXPECT(with_flows(two, {F(0), F(1)}, halo != 0).field_k == 0);
                    EXPECT(with_flows(two, {F(1)}, halo != 0).field_k == 0);
                }
}

void check_closed_k() {
    for (int halo = 0; halo < 2; ++halo)
        for (int steps : {0, 1, 2, 3, mm::kClosedMaxSteps}) {
            mm::PlanIn in = slab(130, 257, 1, 0, 1, halo != 0);
            in.knobs.closed_steps = steps;
            in.knobs.field_steps = in.knobs.field_halo = 4;  // not a closed program's knobs
            const mm::PlanIn alone = with_flows(in, {C(0)}, halo != 0);
            EXPECT(alone.closed_k == ((!halo && steps >= 2) ? steps : 0) && alone.field_k == 0);
            EXPECT(alone.closed_k == mm::closed_k_for(alone, halo != 0));
            for (const Flows& f : {Flows{C(0), C(0)}, Flows{T(0, -1), C(0)}, Flows{C(0), D(0)},
                                   Flows{F(0), C(0)}, Flows{F(0)}, Flows{D(0)}, Flows{}})
                EXPECT(with_flows(in, f, halo != 0).closed_k == 0);
            mm::PlanIn two = in;
            two.n_attr = 2;
            EXPECT(with_flows(two, {C(0)}, halo != 0).closed_k == 0);
            EXPECT(with_flows(two, {C(1)}, halo != 0).closed_k == 0);
        }
    mm::PlanIn off = slab(130, 257, 1, 0, 1, false);
    off.knobs = knobs_of({{"MM_CLOSED_STEPS", "3"}, {"MM_PASSK", "0"}});
    EXPECT(with_flows(off, {C(0)}, false).closed_k == 0);
}

bool parse_flow(const char* s, int n_attr, mm::Flow& f) {
    const size_t n = std::strlen(s);
    auto attr = [&](char c) { return c >= '0' && c < '0' + n_attr ? c - '0' : -1; };
    if (n == 2 && attr(s[1]) >= 0 && (s[0] == 'D' || s[0] == 'F' || s[0] == 'C')) {
        f = s[0] == 'D' ? D(attr(s[1])) : (s[0] == 'F' ? F(attr(s[1])) : C(attr(s[1])));
        return true;
    }
    if (n == 3 && s[0] == 'T' && attr(s[1]) >= 0 && attr(s[2]) >= 0) {
        f = T(attr(s[1]), attr(s[2]));
        return true;
    }
    return false;
}

int print(int argc, char** argv) {
    if (argc < 5) return 2;
    const long long H = std::atoll(argv[2]), W = std::atoll(argv[3]);
    const int n_attr = std::atoi(argv[4]);
    if (H <= 0 || W <= 0 || n_attr < 1 || n_attr > mm::kMaxAttr) return 2;
    std::map<std::string, std::string> env;
    Flows flows;
    for (int i = 5; i < argc; ++i) {
        mm::Flow f;
        if (const char* eq = std::strchr(argv[i], '='))
            env[std::string(argv[i], eq - argv[i])] = eq + 1;
        else if (parse_flow(argv[i], n_attr, f))
            flows.push_back(f);
        else
            return 2;
    }
    mm::PlanIn in = slab(H, W, 1, 0, n_attr, false);
    in.knobs = knobs_of(env);
    in.slots6 = [](int) { return 1; };  // the engine has the six-column instance
    in = with_flows(in, flows, false);
    const mm::SlabPlan sp = mm::slab_plan(in);
    std::printf("%d %d %d |", in.n_passes, (int)sp.kernel, sp.steps_per_launch);
    for (int l : mm::pass_lengths(in, 7)) std::printf(" %d", l);
    std::printf(" |");
    for (int k : kPrintK) {
        const mm::KernelChoice kc = mm::kernel_for(in, k);
        std::printf(" %d %d %lld", (int)kc.kernel, kc.cols, kc.strips);
    }
    std::printf("\n");
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "print") == 0) return print(argc, argv);
    check_passes();
    check_ring();
    check_shape_and_rows();
    check_field_k();
    check_closed_k();
    if (!g_failed) std::printf("ok\n");
    return g_failed;
}
