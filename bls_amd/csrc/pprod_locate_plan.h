// pprod_locate_plan.h -- the host plan of the randomised pairing-product batches that find the bad items by blocks (blsmi 0.18:
// blsmi_pairing_product_batch_rlc_locate*; host only, no HIP, so that tests/native/pprod_locate_plan.cc runs it natively).  Over
// pprod_rlc_plan.h (item_of and the compacted table, as 0.17 has them) the m items are cut into B = ceil(m / block) contiguous blocks, the
// last one possibly shorter; the items of a block are contiguous, so its pairs are one contiguous range.  A CELL is (block b, compacted
// table entry c) with at least one pair of block b referring to c: the unit that is summed and gets a Miller loop.  Cells are of two kinds,
// as 0.17's groups are --
//   multi-pair cells   segments of a permutation of their pairs (the weighted segmented sum's idx), pairs in input order, and
//   one-pair cells     a list of pairs (one 64-bit ladder on one lane each: 0.17's singleton by-pass, now per cell)
// -- and every cell has a SLOT in block order: the cells of block b are adjacent (ascending compacted entry), blocks ascend, slot_off has
// the B + 1 borders.  The sums land multi-pair cells first, then one-pair cells (cell index: multi i -> i, single t -> multi() + t); the
// route kernel moves cell sum_of[s] and table record entry_at[s] to slot s.  q_idx == NULL is the no-sort identity: every pair is a
// one-pair cell and slot = pair = entry.  block >= m gives one block whose cells are 0.17's groups in 0.17's order.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "group_plan.h"
#include "pprod_rlc_plan.h"

namespace blsmi_route {

// block == 0 in a call: max(64, ceil(m / 256)).  Any value >= 1 is legal: every cell has a Miller loop of its own, no layout pairs two cells.
inline size_t pprod_locate_auto_block(size_t m) { return std::max<size_t>(64, m / 256 + (m % 256 != 0)); }

struct PprodLocatePlan {
    size_t m = 0, block = 0;
    std::vector<uint32_t> item_of;    // np: the item of pair k
    std::vector<uint32_t> entry_of;   // d': the table entry of compacted entry c (0.17's numbering)
    std::vector<uint32_t> group_of;   // np: the compacted entry of pair k
    std::vector<uint32_t> perm;       // the pairs of the multi-pair cells; cell i is perm[cell_off[i] .. cell_off[i + 1])
    std::vector<uint64_t> cell_off;   // multi() + 1 offsets into perm, from 0, each step >= 2
    std::vector<uint32_t> single;     // the pair of every one-pair cell
    std::vector<uint32_t> sum_of;     // C: the cell index whose sum goes to slot s
    std::vector<uint32_t> entry_at;   // C: the compacted entry of the cell at slot s
    std::vector<uint64_t> slot_off;   // B + 1 offsets into the slots, from 0 to C, non-decreasing (a block may have no cell)
    size_t blocks() const { return slot_off.size() - 1; }
    size_t multi() const { return cell_off.size() - 1; }
    size_t cells() const { return sum_of.size(); }
    size_t item_lo(size_t b) const { return b * block; }                   // (b < blocks(): b * block < m, no overflow)
    size_t item_hi(size_t b) const { return m - b * block > block ? b * block + block : m; }
};
// false: what pprod_rlc_plan refuses (the plan is then unspecified).  block >= 1 (the caller has resolved 0).  m == 0 gives no block.
inline bool pprod_locate_plan(const uint64_t* seg_off, size_t m, const uint32_t* q_idx, size_t np, size_t nq, size_t block, PprodLocatePlan& p) {
    p.m = m; p.block = block;
    p.perm.clear(); p.single.clear(); p.sum_of.clear(); p.entry_at.clear();
    p.cell_off.assign(1, 0); p.slot_off.assign(1, 0);
    PprodRlcPlan base;
    if (block == 0 || !pprod_rlc_plan(seg_off, m, q_idx, np, nq, base)) return false;
    p.item_of.swap(base.item_of); p.entry_of.swap(base.entry_of); p.group_of.swap(base.group_of);
    const size_t B = m / block + (m % block != 0);
    p.slot_off.reserve(B + 1);
    if (!q_idx) {                                                          // the identity: slot = pair = entry, every cell a one-pair cell
        p.single = p.entry_of; p.sum_of = p.entry_of; p.entry_at = p.entry_of;
        for (size_t b = 0; b < B; b++) p.slot_off.push_back(seg_off[p.item_hi(b)]);
        return true;
    }
    // pass 1, block by block: the entries its pairs touch, counted; ascending, they are the block's cells
    const size_t dg = p.entry_of.size();
    std::vector<uint32_t> count(dg, 0), touched, kind_at;                  // kind_at[s]: 1 = the cell at slot s is a multi-pair cell
    std::vector<uint64_t> start(dg, 0);                                    // compacted entry -> where its cell's next pair goes in perm
    std::vector<uint32_t> multi_pairs;                                     // per multi-pair cell, in order: its number of pairs
    size_t nmulti = 0, nsingle = 0;
    for (size_t b = 0; b < B; b++) {
        touched.clear();
        for (uint64_t k = seg_off[p.item_lo(b)]; k < seg_off[p.item_hi(b)]; k++) if (count[p.group_of[k]]++ == 0) touched.push_back(p.group_of[k]);
        std::sort(touched.begin(), touched.end());
        for (uint32_t c : touched) {
            const bool mu = count[c] >= 2;
            p.entry_at.push_back(c); kind_at.push_back(mu ? 1 : 0);
            p.sum_of.push_back((uint32_t)(mu ? nmulti++ : nsingle++));     // (one-pair cells: shifted behind the multi-pair cells below)
            if (mu) { multi_pairs.push_back(count[c]); p.cell_off.push_back(p.cell_off.back() + count[c]); }
            count[c] = 0;
        }
        p.slot_off.push_back(p.sum_of.size());
    }
    for (size_t s = 0; s < p.sum_of.size(); s++) if (!kind_at[s]) p.sum_of[s] += (uint32_t)nmulti;
    // pass 2: the pairs into their cells, in input order
    p.perm.resize((size_t)p.cell_off.back()); p.single.resize(nsingle);
    for (size_t b = 0; b < B; b++) {
        for (uint64_t s = p.slot_off[b]; s < p.slot_off[b + 1]; s++) {
            const uint32_t c = p.entry_at[s];
            if (kind_at[s]) { start[c] = p.cell_off[p.sum_of[s]]; count[c] = 1; }
            else { start[c] = p.sum_of[s] - nmulti; count[c] = 0; }
        }
        for (uint64_t k = seg_off[p.item_lo(b)]; k < seg_off[p.item_hi(b)]; k++) {
            const uint32_t c = p.group_of[k];
            if (count[c]) p.perm[start[c]++] = (uint32_t)k;
            else p.single[start[c]] = (uint32_t)k;
        }
    }
    return true;
}

// x further cells behind the own cells of EVERY block, whose sums the weighted sums do not make (blsmi 0.19: a Groth16 batch's alpha and
// gamma cells, folded in the scalar field): cell i of block b takes sum index C + i * B + b, C the cells before the call, and compacted
// entry d' + i, where entries[i] joins entry_of.  The pairs, their permutation and the one-pair list stay as they are.
inline void pprod_locate_append_cells(PprodLocatePlan& p, const uint32_t* entries, size_t x) {
    const size_t B = p.blocks(), C = p.cells(), dg = p.entry_of.size();
    std::vector<uint32_t> sum_of, entry_at;
    std::vector<uint64_t> slot_off(1, 0);
    sum_of.reserve(C + x * B); entry_at.reserve(C + x * B); slot_off.reserve(B + 1);
    for (size_t b = 0; b < B; b++) {
        for (uint64_t s = p.slot_off[b]; s < p.slot_off[b + 1]; s++) { sum_of.push_back(p.sum_of[s]); entry_at.push_back(p.entry_at[s]); }
        for (size_t i = 0; i < x; i++) { sum_of.push_back((uint32_t)(C + i * B + b)); entry_at.push_back((uint32_t)(dg + i)); }
        slot_off.push_back(sum_of.size());
    }
    p.entry_of.insert(p.entry_of.end(), entries, entries + x);
    p.sum_of.swap(sum_of); p.entry_at.swap(entry_at); p.slot_off.swap(slot_off);
}

// What the recheck of the failing blocks reads, given one byte per block (not zero: the block's value was not one), everything ascending:
struct PprodLocateFailing {
    std::vector<uint32_t> items;      // the items of the failing blocks: where the dense verdicts are scattered to
    std::vector<uint32_t> pairs;      // their pairs: the gathers of the G1 records and of the flag bytes
    std::vector<uint32_t> entries;    // as long as pairs: the compacted entry of each, the gather of the table records (group_of composed here)
    std::vector<uint64_t> dense_off;  // items.size() + 1 offsets of the dense items over the dense pairs, from 0
};
inline void pprod_locate_failing(const PprodLocatePlan& p, const uint64_t* seg_off, const uint8_t* fail, PprodLocateFailing& f) {
    f.items.clear(); f.pairs.clear(); f.entries.clear();
    f.dense_off.assign(1, 0);
    for (size_t b = 0; b < p.blocks(); b++) {
        if (!fail[b]) continue;
        for (size_t j = p.item_lo(b); j < p.item_hi(b); j++) {
            f.items.push_back((uint32_t)j);
            f.dense_off.push_back(f.dense_off.back() + (seg_off[j + 1] - seg_off[j]));
        }
        for (uint64_t k = seg_off[p.item_lo(b)]; k < seg_off[p.item_hi(b)]; k++) { f.pairs.push_back((uint32_t)k); f.entries.push_back(p.group_of[k]); }
    }
}

}  // namespace blsmi_route
