// pprod_locate_append_cells of bls_amd/csrc/pprod_locate_plan.h on the host (tests/test_groth16_cpu.py compiles this with the address and
// undefined-behaviour sanitizers): the plan of a Groth16 batch -- m items of two pairs, (A_j, entry j) and (C_j, entry m) -- at the block
// size argv[2], with two further cells per block appended.  Checks the invariants the drivers rely on and prints the slots.
//   pprod_locate_append m block
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../bls_amd/csrc/pprod_locate_plan.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "check failed: %s (line %d)\n", #x, __LINE__); return 1; } } while (0)

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: pprod_locate_append m block\n"); return 2; }
    const size_t m = strtoull(argv[1], nullptr, 10), block = strtoull(argv[2], nullptr, 10);
    std::vector<uint64_t> seg_off(m + 1);
    std::vector<uint32_t> q_idx(2 * m);
    for (size_t j = 0; j < m; j++) { seg_off[j] = 2 * j; q_idx[2 * j] = (uint32_t)j; q_idx[2 * j + 1] = (uint32_t)m; }
    seg_off[m] = 2 * m;
    blsmi_route::PprodLocatePlan before, p;
    CHECK(blsmi_route::pprod_locate_plan(seg_off.data(), m, q_idx.data(), 2 * m, m + 1, block, before));
    p = before;
    const uint32_t further[2] = {(uint32_t)(m + 1), (uint32_t)(m + 2)};
    blsmi_route::pprod_locate_append_cells(p, further, 2);
    const size_t B = before.blocks(), C = before.cells(), dg = before.entry_of.size();
    CHECK(p.blocks() == B && p.cells() == C + 2 * B && p.entry_of.size() == dg + 2);
    CHECK(p.entry_of[dg] == m + 1 && p.entry_of[dg + 1] == m + 2);
    CHECK(p.perm == before.perm && p.single == before.single && p.cell_off == before.cell_off && p.group_of == before.group_of && p.item_of == before.item_of);
    std::vector<int> seen(p.cells(), 0);
    for (size_t b = 0; b < B; b++) {
        const uint64_t lo = p.slot_off[b], hi = p.slot_off[b + 1], own = before.slot_off[b + 1] - before.slot_off[b];
        CHECK(hi - lo == own + 2);
        for (uint64_t s = 0; s < own; s++) CHECK(p.sum_of[lo + s] == before.sum_of[before.slot_off[b] + s] && p.entry_at[lo + s] == before.entry_at[before.slot_off[b] + s]);
        for (size_t i = 0; i < 2; i++) CHECK(p.sum_of[lo + own + i] == C + i * B + b && p.entry_at[lo + own + i] == dg + i);   // cell-major: every alpha cell, then every gamma cell
        for (uint64_t s = lo; s < hi; s++) { CHECK(p.sum_of[s] < p.cells() && p.entry_at[s] < p.entry_of.size()); seen[p.sum_of[s]]++; }
    }
    for (int n : seen) CHECK(n == 1);                                            // every sum goes to exactly one slot
    printf("sum_of"); for (uint32_t v : p.sum_of) printf(" %u", v);
    printf("\nentry_at"); for (uint32_t v : p.entry_at) printf(" %u", v);
    printf("\nslot_off"); for (uint64_t v : p.slot_off) printf(" %llu", (unsigned long long)v);
    printf("\n");
    return 0;
}
