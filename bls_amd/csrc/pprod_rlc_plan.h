// pprod_rlc_plan.h -- the host plan of the randomised pairing-product batches (blsmi 0.17: blsmi_pairing_product_batch_rlc*; host only, no
// HIP, so that tests/native/pprod_rlc_plan.cc runs it natively).  Pair k of np belongs to item item_of[k] (the items' offsets) and refers to
// entry q_idx[k] of a table of nq G2 points (q_idx null: entry k).  group_plan.h groups the pairs by entry; here its groups are split into
//   shared groups   two or more pairs: their weighted sum goes through the segmented sum (a ladder per pair, folds, a wave per group), and
//   singletons      one pair: one 64-bit ladder on one lane, no wave of its own -- a batch whose G2 points are mostly private (the B_j of
//                   Groth16, q_idx == NULL) would otherwise pay the segmented sum's final pass, one wave per group, np times.
// The compacted groups the Miller loops run over are numbered shared first (in table order), then singletons (in table order).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "group_plan.h"

namespace blsmi_route {

struct PprodRlcPlan {
    std::vector<uint32_t> item_of;    // np: the item of pair k
    std::vector<uint32_t> perm;       // the pairs of the shared groups; shared group g is perm[seg_off[g] .. seg_off[g + 1]), in input order
    std::vector<uint64_t> seg_off;    // shared + 1 offsets into perm, from 0, each step >= 2
    std::vector<uint32_t> single;     // the pair of every singleton group
    std::vector<uint32_t> entry_of;   // d' = shared + singletons: the table entry of compacted group c
    std::vector<uint32_t> group_of;   // np: the compacted group of pair k
    size_t shared() const { return seg_off.size() - 1; }
    size_t groups() const { return entry_of.size(); }
};
// offsets of m items over np pairs: from 0, non-decreasing, ending at np
inline bool pprod_rlc_offsets_valid(const uint64_t* seg_off, size_t m, size_t np) {
    if (!seg_off || seg_off[0] != 0) return false;
    for (size_t j = 0; j < m; j++) if (seg_off[j + 1] < seg_off[j]) return false;
    return seg_off[m] == np;
}
// false: bad offsets, some q_idx[k] >= nq, q_idx null with nq != np, or np beyond 32 bits (the plan is then unspecified).
// split == false sends every group through the segmented sum (the measurement of the singleton by-pass).
inline bool pprod_rlc_plan(const uint64_t* seg_off, size_t m, const uint32_t* q_idx, size_t np, size_t nq, PprodRlcPlan& p, bool split = true) {
    p.item_of.clear(); p.perm.clear(); p.single.clear(); p.entry_of.clear(); p.group_of.clear();
    p.seg_off.assign(1, 0);
    if (np > 0xffffffffull || !pprod_rlc_offsets_valid(seg_off, m, np)) return false;
    if (!q_idx && nq != np) return false;
    p.item_of.resize(np);
    for (size_t j = 0; j < m; j++) for (uint64_t k = seg_off[j]; k < seg_off[j + 1]; k++) p.item_of[k] = (uint32_t)j;
    if (!q_idx) {                                                          // every pair its own entry: the identity, without the sort
        p.group_of.resize(np); p.entry_of.resize(np);
        for (size_t k = 0; k < np; k++) p.group_of[k] = p.entry_of[k] = (uint32_t)k;
        if (split) p.single = p.entry_of;
        else { p.perm = p.entry_of; for (size_t k = 0; k < np; k++) p.seg_off.push_back(k + 1); }
        return true;
    }
    GroupPlan gp;
    if (!group_plan(q_idx, np, nq, gp)) return false;
    const size_t dg = gp.msg_of.size();
    auto is_shared = [&](size_t g) { return !split || gp.seg_off[g + 1] - gp.seg_off[g] >= 2; };
    std::vector<uint32_t> compact(dg);                                     // group_plan's group -> compacted group
    size_t nsh = 0;
    for (size_t g = 0; g < dg; g++) nsh += is_shared(g);
    p.entry_of.resize(dg);
    size_t sh = 0, si = nsh;
    for (size_t g = 0; g < dg; g++) {
        const size_t c = is_shared(g) ? sh++ : si++;
        compact[g] = (uint32_t)c;
        p.entry_of[c] = gp.msg_of[g];
        if (is_shared(g)) {
            p.perm.insert(p.perm.end(), gp.perm.begin() + gp.seg_off[g], gp.perm.begin() + gp.seg_off[g + 1]);
            p.seg_off.push_back(p.perm.size());
        } else p.single.push_back(gp.perm[gp.seg_off[g]]);
    }
    p.group_of.resize(np);
    for (size_t k = 0; k < np; k++) p.group_of[k] = compact[gp.group_of[k]];
    return true;
}

}  // namespace blsmi_route
