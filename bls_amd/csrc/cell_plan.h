// cell_plan.h -- the host plan of the grouped randomised verification that finds the bad tuples by cells (blsmi 0.13:
// blsmi_g?pubs_*verify*_batch_rlc_grouped_locate; host only, no HIP, so that tests/native/cell_plan.cc runs it natively).  group_plan.h has
// sorted the tuples by message; every non-empty group is cut here, in the order of its permutation, into cells of at most `block`
// consecutive positions: in each group every cell but the last is full, and no cell crosses a group border.  A cell is the unit of the
// call's sums (keys and signatures), of its Miller loops and of the equations that decide which tuples are verified one by one.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "group_plan.h"

namespace blsmi_route {

struct CellPlan {
    size_t block = 0;
    std::vector<uint64_t> cell_off;   // C + 1 offsets into GroupPlan::perm, from 0 to n, strictly increasing (no cell is empty)
    std::vector<uint32_t> group_of;   // C: the group of cell c (its hash point is that group's)
    size_t cells() const { return cell_off.size() - 1; }
};
// block >= 1 (the caller has resolved 0: locate_plan.h, locate_auto_block); block >= a group's size leaves the group whole.  The empty plan
// (n == 0) gives no cell.
inline void cell_plan(const GroupPlan& g, size_t block, CellPlan& p) {
    p.block = block;
    p.cell_off.assign(1, 0); p.group_of.clear();
    for (size_t j = 0; j + 1 < g.seg_off.size(); j++) {
        const uint64_t hi = g.seg_off[j + 1];
        for (uint64_t lo = g.seg_off[j]; lo < hi;) {
            lo = hi - lo > block ? lo + block : hi;
            p.cell_off.push_back(lo);
            p.group_of.push_back((uint32_t)j);
        }
    }
}
// The tuples of the cells whose byte in `fail` is not zero, cell after cell in the order of the permutation -- pos: their positions in the
// call (what the per-tuple stage gathers keys, signatures and flags by, and scatters its verdicts to), grp: the group of each (what it
// gathers the hash points by).
inline void cell_positions(const GroupPlan& g, const CellPlan& p, const uint8_t* fail, std::vector<uint32_t>& pos, std::vector<uint32_t>& grp) {
    pos.clear(); grp.clear();
    for (size_t c = 0; c < p.cells(); c++)
        if (fail[c]) for (uint64_t k = p.cell_off[c]; k < p.cell_off[c + 1]; k++) { pos.push_back(g.perm[k]); grp.push_back(p.group_of[c]); }
}

}  // namespace blsmi_route
