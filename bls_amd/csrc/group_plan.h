// group_plan.h -- the host plan of the grouped randomised verification (blsmi 0.11: blsmi_g?pubs_*verify*_batch_rlc_grouped; host only, no
// HIP, so that tests/native/group_plan.cc runs it natively).  Tuple i of n refers to message msg_idx[i] of a table of d.  A counting sort of
// the tuples by msg_idx gives the permutation the weighted segmented sum reads as its `idx` (the tuples of one message are contiguous in it,
// in their input order); messages no tuple refers to take no part: the d' non-empty groups are numbered in table order.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace blsmi_route {

struct GroupPlan {
    std::vector<uint32_t> perm;      // n: the tuples sorted by message; group g is perm[seg_off[g] .. seg_off[g + 1])
    std::vector<uint64_t> seg_off;   // d' + 1 offsets into perm, from 0, strictly increasing (no group is empty)
    std::vector<uint32_t> msg_of;    // d': the table entry of group g
    std::vector<uint32_t> group_of;  // n: the group of tuple i (the per-tuple path gathers its hash point by this)
};
// false: some msg_idx[i] >= d (the plan is then unspecified); n == 0 gives the empty plan (seg_off = {0})
inline bool group_plan(const uint32_t* msg_idx, size_t n, size_t d, GroupPlan& p) {
    p.perm.clear(); p.msg_of.clear(); p.group_of.clear();
    p.seg_off.assign(1, 0);
    if (n == 0) return true;
    std::vector<uint64_t> count(d, 0);
    for (size_t i = 0; i < n; i++) {
        if (msg_idx[i] >= d) return false;
        count[msg_idx[i]]++;
    }
    std::vector<uint32_t> group(d, 0);                                     // table entry -> group (entries with count 0: unused)
    std::vector<uint64_t> next(d, 0);                                      // table entry -> where its next tuple goes
    for (size_t j = 0; j < d; j++) {
        if (count[j] == 0) continue;
        group[j] = (uint32_t)p.msg_of.size();
        next[j] = p.seg_off.back();
        p.msg_of.push_back((uint32_t)j);
        p.seg_off.push_back(p.seg_off.back() + count[j]);
    }
    p.perm.resize(n); p.group_of.resize(n);
    for (size_t i = 0; i < n; i++) {
        const uint32_t j = msg_idx[i];
        p.perm[next[j]++] = (uint32_t)i;
        p.group_of[i] = group[j];
    }
    return true;
}

}  // namespace blsmi_route
