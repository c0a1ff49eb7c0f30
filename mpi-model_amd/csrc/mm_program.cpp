// mm_program.cpp -- flow programs for the planner (mm_program.hpp).
#include "mm_program.hpp"

#include "../../include/mpimodel.h"

namespace mm {

std::vector<Pass> compile_passes(const std::vector<Flow>& flows) {
    std::vector<Pass> passes;
    Pass cur;
    bool open = false;
    for (const Flow& f : flows) {
        // a closed diffusion is a pass of its own: it closes any open pass and shares its
        // own with nothing
        if (f.kind == MM_FLOW_DIFFUSE_CLOSED) {
            if (open) passes.push_back(cur);
            open = false;
            Pass c;
            c.field_mask = 1 << f.a;
            c.closed = true;
            passes.push_back(c);
            continue;
        }
        // rate-field diffusions get passes of their own: consecutive ones of distinct
        // attributes share a pass; any other flow closes it, and they close any other pass
        const bool fieldf = f.kind == MM_FLOW_DIFFUSE_FIELD;
        if (open && (fieldf ? (!cur.field_mask || (cur.field_mask & (1 << f.a))) : cur.field_mask != 0)) {
            passes.push_back(cur);
            open = false;
        }
        if (fieldf) {
            if (!open) {
                cur = Pass();
                open = true;
            }
            cur.field_mask |= 1 << f.a;
        } else if (f.kind == MM_FLOW_TRANSFER) {
            if (!open) {
                cur = Pass();
                open = true;
            }
            std::vector<Transfer>& chain = cur.diffuse_mask ? cur.post : cur.pre;
            if ((int)chain.size() >= kMaxChain) {
                passes.push_back(cur);
                cur = Pass();
                cur.pre.push_back({f.a, f.b, f.rate});
            } else {
                chain.push_back({f.a, f.b, f.rate});
            }
        } else {  // MM_FLOW_DIFFUSE
            if (!open) {
                cur = Pass();
                open = true;
            }
            if ((cur.diffuse_mask & (1 << f.a)) || !cur.post.empty()) {
                passes.push_back(cur);
                cur = Pass();
            }
            cur.diffuse_mask |= 1 << f.a;
            cur.drate[f.a] = f.rate;
        }
    }
    if (open) passes.push_back(cur);
    return passes;
}

bool ring_program(const Knobs& knobs, int n_attr, const std::vector<Pass>& passes) {
    if (!knobs.ring_ok || n_attr != 4 || passes.size() != 1) return false;
    const Pass& p = passes[0];
    if ((int)p.pre.size() != n_attr || !p.post.empty() || p.diffuse_mask != 15) return false;
    for (int t = 0; t < n_attr; ++t)
        if (p.pre[t].a != t || p.pre[t].b != (t + 1) % n_attr) return false;
    return true;
}

void set_program(PlanIn& pin, const std::vector<Pass>& passes, bool halo, int th_env) {
    const int na = pin.n_attr;
    pin.n_passes = (int)passes.size();
    const Pass* p = pin.n_passes == 1 ? &passes[0] : nullptr;
    pin.diffuse_mask = p ? p->diffuse_mask : 0;
    pin.chains = p && !(p->pre.empty() && p->post.empty());
    pin.ring = ring_program(pin.knobs, na, passes);
    pin.field = pin.closed = false;
    for (const Pass& q : passes) {
        pin.field = pin.field || q.field_mask != 0;
        pin.closed = pin.closed || q.closed;  // one step per pass, whatever the knobs say
    }
    // transfers, several attributes or a rate field: those kernels exist for 8-row blocks
    // only. Any other program, the empty one included, gets the height the environment asked
    // for back: a reprogrammed engine plans as a fresh one (include/mpimodel.h, mm_clear_flows)
    bool eight = na > 1;
    for (const Pass& q : passes)
        eight = eight || !q.pre.empty() || !q.post.empty() || q.field_mask != 0;
    pin.knobs.th = eight ? 8 : th_env;
    // K-step rate-field passes (mm_fieldk_kernel): one attribute and a program that is
    // exactly one field diffusion (further attributes would need a copy). With a halo -- a
    // chain, a self-halo, any halo mode -- K is also bounded by the ghost rows of the field
    // the caller promised at creation (MM_FIELD_HALO, 1 unless set: one step per pass) and by
    // the chain's thinnest slab; whether the rows are there is the engine's business (check_run).
    const bool alone = na == 1 && p && p->field_mask == 1 && !p->closed && p->diffuse_mask == 0 &&
                       !pin.chains;
    pin.field_k = alone ? field_k_for(pin, halo) : 0;
    // K-step closed passes (mm_closedk_kernel): one attribute, a program that is exactly one
    // closed diffusion, and MM_CLOSED_STEPS asking for them; with a halo K + 1 promised ghost
    // rows of the field as well (MM_CLOSED_HALO) and a chain no thinner than K
    const bool closed_alone = na == 1 && p && p->field_mask == 1 && p->closed;
    pin.closed_k = closed_alone ? closed_k_for(pin, halo) : 0;
}

}  // namespace mm
