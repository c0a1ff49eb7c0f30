// mm_program.hpp -- a flow program, from the list mm_add_flow builds to what the planner sees
// of it: the flows grouped into fused passes, the C5 ring recognised, and the program's shape
// written into mm::PlanIn (mm_plan.hpp). Host-only like the planner: no HIP, no engine;
// mm_engine.hip keeps the flow list and calls this, tests/program_cli.cpp checks it without a
// GPU.
#pragma once

#include <vector>

#include "mm_plan.hpp"

namespace mm {

// One mm_add_flow call: kind is an MM_FLOW_* of include/mpimodel.h, b the target of a
// transfer (-1: none).
struct Flow {
    int kind, a, b;
    double rate;
};

struct Transfer {
    int a, b;
    double rate;
};

// A fused pass: pre-chain transfers, at most one diffusion per attribute, post-chain. A
// rate-field pass (field_mask != 0) holds field diffusions of distinct attributes only.
struct Pass {
    std::vector<Transfer> pre, post;
    int diffuse_mask = 0;
    double drate[kMaxAttr] = {0, 0, 0, 0};
    int field_mask = 0;
    // a closed rate-field diffusion (MM_FLOW_DIFFUSE_CLOSED, mm_closed_kernel): the pass holds
    // that one flow alone, field_mask its attribute's bit
    bool closed = false;
};

// The passes of one step, in the flows' order.
std::vector<Pass> compile_passes(const std::vector<Flow>& flows);

// A one-pass program of four attributes whose pre-chain is the ring of transfers t -> t+1
// mod 4 in that order, without a post-chain (config C5's topology), runs the wide instance
// with the chain's operands fixed at compile time.
bool ring_program(const Knobs& knobs, int n_attr, const std::vector<Pass>& passes);

// The program's shape, for the planner: n_passes, diffuse_mask, chains, ring, field, closed,
// the effective knobs.th, field_k and closed_k of `in`, whose slab, attribute count and other
// knobs are already set. halo: the slab has one (a neighbour, or a halo mode on one slab, the
// self-halo among them). th_env: MM_ROWS_PER_WAVE as the environment asked.
void set_program(PlanIn& in, const std::vector<Pass>& passes, bool halo, int th_env);

}  // namespace mm
