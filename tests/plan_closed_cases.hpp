// plan_closed_cases.hpp -- the programs the engine knew before the closed kind, on the slabs
// whose plans tests/plan_closed_table.inc recorded then (`plan_closed_cli table` of the planner
// of that commit), for plan_closed_cli.cpp and plan_closedk_cli.cpp. Each program is a real
// flow list, described to the planner by mm::compile_passes and mm::set_program.
#pragma once

#include "plan_test.hpp"

namespace {

enum Program { kDiffuse, kC5, kField, kFieldAlone, kThreePasses };
const char* const kProgramNames[] = {"diffuse", "c5", "field", "field_alone", "three_passes"};

mm::PlanIn program(const mm::PlanIn& in, Program p, bool halo) {
    switch (p) {
        case kDiffuse:
            return with_flows(in, {D(0)}, halo);
        case kC5:
            return with_flows(in, {T(0, 1), T(1, 2), T(2, 3), T(3, 0), D(0), D(1), D(2), D(3)}, halo);
        case kField:       // a field pass on an engine of several attributes: one step per pass
        case kFieldAlone:  // exactly one field diffusion, one attribute: K-step passes
            return with_flows(in, {F(0)}, halo);
        case kThreePasses:
            return with_flows(in, {D(0), D(0), D(0)}, halo);
    }
    return in;
}

struct Case {
    long long H, W;
    int G, g, n_attr;
    bool split;
    Program p;
    int field_steps, field_halo;
};

const Case kCases[] = {
    {130, 97, 1, 0, 1, false, kDiffuse, 0, 1},      {2048, 2048, 1, 0, 1, false, kDiffuse, 0, 1},
    {8192, 8192, 1, 0, 1, false, kDiffuse, 0, 1},   {32768, 32768, 1, 0, 1, false, kDiffuse, 4, 4},
    {32768, 32768, 8, 3, 1, true, kDiffuse, 0, 1},  {4096, 4096, 1, 0, 4, false, kC5, 0, 1},
    {67, 300, 3, 1, 4, true, kC5, 4, 4},            {130, 257, 1, 0, 3, false, kField, 4, 4},
    {27, 257, 3, 1, 2, true, kField, 0, 2},         {130, 257, 1, 0, 1, false, kFieldAlone, 0, 1},
    {2048, 2048, 1, 0, 1, false, kFieldAlone, 0, 1}, {8192, 8192, 1, 0, 1, false, kFieldAlone, 3, 1},
    {8192, 8192, 1, 0, 1, true, kFieldAlone, 0, 4}, {8192, 8192, 1, 0, 1, true, kFieldAlone, 4, 1},
    {27, 257, 3, 1, 1, true, kFieldAlone, 4, 4},    {4096, 2048, 2, 1, 1, true, kFieldAlone, 0, 4},
    {130, 97, 1, 0, 3, false, kThreePasses, 4, 4},  {8192, 8192, 2, 0, 2, true, kThreePasses, 0, 1},
};

// closed_steps: MM_CLOSED_STEPS, which no program here reads.
mm::PlanIn case_in(const Case& c, int closed_steps = 0) {
    mm::PlanIn in = slab(c.H, c.W, c.G, c.g, c.n_attr, c.split);
    in.knobs.field_steps = c.field_steps;
    in.knobs.field_halo = c.field_halo;
    in.knobs.closed_steps = closed_steps;
    return program(in, c.p, c.split);
}

// The case's line of the table.
std::string case_text(const Case& c, int closed_steps = 0) {
    char buf[128];
    std::snprintf(buf, sizeof buf, "%s %lldx%lld %d/%d na%d fs%d fh%d: ", kProgramNames[c.p], c.H, c.W, c.g,
                  c.G, c.n_attr, c.field_steps, c.field_halo);
    return buf + plan_text(case_in(c, closed_steps));
}

const char* const kTable[] = {
#include "plan_closed_table.inc"
};
constexpr size_t kNCases = sizeof kCases / sizeof kCases[0];

// Every case still prints its recorded line.
void check_table(int closed_steps = 0) {
    EXPECT(sizeof kTable / sizeof kTable[0] == kNCases);
    for (size_t i = 0; i < kNCases && i < sizeof kTable / sizeof kTable[0]; ++i)
        if (case_text(kCases[i], closed_steps) != kTable[i]) {
            std::printf("plan changed:\n  was %s\n  is  %s\n", kTable[i],
                        case_text(kCases[i], closed_steps).c_str());
            g_failed = 1;
        }
}

}  // namespace
