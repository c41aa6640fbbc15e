// Driver of bls_amd/csrc/pprod_locate_plan.h (over pprod_rlc_plan.h and group_plan.h) for tests/test_pprod_rlc_locate_cpu.py (built with
// -fsanitize=address,undefined).  Without arguments: fixed and pseudo-random cases, each checked here against a brute-force restatement --
// item_of, entry_of and group_of are 0.17's; every pair is in exactly one cell; no cell crosses a block or an entry and no (block, entry)
// has two cells; a cell of two or more pairs is a segment of perm in input order, every other one an element of `single`; the slots are a
// permutation of the cells grouped by ascending block and, inside a block, ascending entry; slot_off has B + 1 borders; block >= m
// reproduces 0.17's grouping; the failing-block listings for none, all, only the last, and a pseudo-random choice.  Prints
// "PPROD_LOCATE_PLAN ok <cases>".  With arguments `block nq m off0 .. offm [q0 q1 ...]` (no q: q_idx NULL): prints the plan or "invalid".
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

#include "../../bls_amd/csrc/pprod_locate_plan.h"

using blsmi_route::PprodLocateFailing;
using blsmi_route::PprodLocatePlan;
using blsmi_route::PprodRlcPlan;
using blsmi_route::pprod_locate_failing;
using blsmi_route::pprod_locate_plan;
using blsmi_route::pprod_rlc_plan;

static int fail(const char* what, const char* name, size_t block) {
    printf("PPROD_LOCATE_PLAN FAILED %s (block %zu): %s\n", name, block, what);
    return 1;
}

static int check_failing(const char* name, const PprodLocatePlan& p, const std::vector<uint64_t>& off, const std::vector<uint8_t>& bytes) {
    PprodLocateFailing f;
    pprod_locate_failing(p, off.data(), bytes.data(), f);
    const size_t m = off.size() - 1;
    std::vector<uint32_t> items, pairs;
    std::vector<uint64_t> dense{0};
    for (size_t j = 0; j < m; j++) {
        if (!bytes[j / p.block]) continue;
        items.push_back((uint32_t)j);
        for (uint64_t k = off[j]; k < off[j + 1]; k++) pairs.push_back((uint32_t)k);
        dense.push_back(pairs.size());
    }
    if (f.items != items) return fail("failing items", name, p.block);
    if (f.pairs != pairs) return fail("failing pairs", name, p.block);
    if (f.dense_off != dense) return fail("dense offsets", name, p.block);
    if (f.entries.size() != pairs.size()) return fail("failing entries' size", name, p.block);
    for (size_t r = 0; r < pairs.size(); r++) if (f.entries[r] != p.group_of[pairs[r]]) return fail("failing entries", name, p.block);
    return 0;
}

static int check(const char* name, const std::vector<uint64_t>& off, const std::vector<uint32_t>* q, size_t nq, size_t block, bool want_ok) {
    PprodLocatePlan p;
    PprodRlcPlan base;
    const size_t m = off.size() - 1, np = (size_t)off.back() < ((size_t)1 << 24) ? (size_t)off.back() : 0;
    const size_t npairs = q ? q->size() : np;
    static const uint32_t none = 0;                                         // (an empty vector's data() may be null, which would say "no q_idx")
    const uint32_t* qp = q ? (q->empty() ? &none : q->data()) : nullptr;
    const bool ok = pprod_locate_plan(off.data(), m, qp, npairs, nq, block, p);
    if (ok != want_ok) return fail("verdict", name, block);
    if (!ok) return 0;
    if (!pprod_rlc_plan(off.data(), m, qp, npairs, nq, base)) return fail("0.17's plan refuses what this one takes", name, block);
    if (p.item_of != base.item_of || p.entry_of != base.entry_of || p.group_of != base.group_of) return fail("item_of / entry_of / group_of are not 0.17's", name, block);
    const size_t B = m / block + (m % block != 0), C = p.cells(), Cm = p.multi(), Cs = p.single.size();
    if (p.m != m || p.block != block || p.blocks() != B) return fail("block count", name, block);
    if (p.entry_at.size() != C || Cm + Cs != C) return fail("cell counts", name, block);
    if (p.cell_off[0] != 0 || p.cell_off[Cm] != p.perm.size() || p.perm.size() + Cs != npairs) return fail("offsets' ends", name, block);
    // brute force: (block, compacted entry) -> its pairs in input order
    std::map<std::pair<size_t, uint32_t>, std::vector<uint32_t>> want;
    for (size_t k = 0; k < npairs; k++) want[{p.item_of[k] / block, p.group_of[k]}].push_back((uint32_t)k);
    if (want.size() != C) return fail("one cell per (block, entry)", name, block);
    // the pairs of every cell, by cell index
    std::vector<std::vector<uint32_t>> cell(C);
    for (size_t i = 0; i < Cm; i++) {
        if (p.cell_off[i + 1] < p.cell_off[i] + 2) return fail("a multi-pair cell of fewer than two pairs", name, block);
        cell[i].assign(p.perm.begin() + p.cell_off[i], p.perm.begin() + p.cell_off[i + 1]);
    }
    for (size_t t = 0; t < Cs; t++) cell[Cm + t].assign(1, p.single[t]);
    std::vector<uint8_t> seen(npairs, 0), used(C, 0);
    for (size_t i = 0; i < C; i++) for (uint32_t k : cell[i]) {
        if (k >= npairs || seen[k]) return fail("a pair twice or out of range", name, block);
        seen[k] = 1;
    }
    for (size_t k = 0; k < npairs; k++) if (!seen[k]) return fail("a pair in no cell", name, block);
    // the slots: a permutation, in the map's order (ascending block, then ascending entry), the borders where the block changes
    if (p.slot_off[0] != 0 || p.slot_off[B] != C) return fail("slot borders' ends", name, block);
    size_t s = 0;
    for (const auto& kv : want) {
        const size_t b = kv.first.first;
        if (b >= B || s < p.slot_off[b] || s >= p.slot_off[b + 1]) return fail("a slot outside its block's borders", name, block);
        const uint32_t ci = p.sum_of[s];
        if (ci >= C || used[ci]) return fail("slots are not a permutation of the cells", name, block);
        used[ci] = 1;
        if (p.entry_at[s] != kv.first.second) return fail("a slot's entry", name, block);
        if (cell[ci] != kv.second) return fail("a cell's pairs (another block's or entry's, or out of input order)", name, block);
        if ((kv.second.size() >= 2) != (ci < Cm)) return fail("a cell of the wrong kind", name, block);
        s++;
    }
    for (size_t b = 0; b < B; b++) if (p.slot_off[b + 1] < p.slot_off[b]) return fail("slot borders decrease", name, block);
    if (!q) for (size_t k = 0; k < npairs; k++) if (p.sum_of[k] != k || p.entry_at[k] != k || p.single[k] != k) return fail("q_idx NULL is not the identity", name, block);
    if (block >= m && m) {                                                  // one block: 0.17's grouping in 0.17's order
        if (p.perm != base.perm || p.cell_off != base.seg_off || p.single != base.single) return fail("block >= m does not reproduce 0.17's groups", name, block);
        for (size_t c = 0; c < C; c++) if (p.sum_of[c] != c || p.entry_at[c] != c) return fail("block >= m: slots out of 0.17's order", name, block);
    }
    // the listings
    int bad = 0;
    std::vector<uint8_t> bytes(B ? B : 1, 0);
    bad += check_failing(name, p, off, bytes);
    for (size_t b = 0; b < B; b++) bytes[b] = 1;
    bad += check_failing(name, p, off, bytes);
    for (size_t b = 0; b + 1 < B; b++) bytes[b] = 0;
    bad += check_failing(name, p, off, bytes);
    uint32_t x = 4242;
    for (size_t b = 0; b < B; b++) { x = x * 1664525u + 1013904223u; bytes[b] = (uint8_t)((x >> 13) % 3 == 0 ? 7 : 0); }
    bad += check_failing(name, p, off, bytes);
    return bad;
}

int main(int argc, char** argv) {
    if (argc > 3) {
        const size_t block = strtoull(argv[1], nullptr, 10), nq = strtoull(argv[2], nullptr, 10), m = strtoull(argv[3], nullptr, 10);
        if ((size_t)argc < 5 + m) return 2;
        std::vector<uint64_t> off;
        for (size_t i = 0; i <= m; i++) off.push_back(strtoull(argv[4 + i], nullptr, 10));
        std::vector<uint32_t> q;
        for (int i = 5 + (int)m; i < argc; i++) q.push_back((uint32_t)strtoul(argv[i], nullptr, 10));
        const bool have_q = (size_t)argc > 5 + m;
        PprodLocatePlan p;
        if (!pprod_locate_plan(off.data(), m, have_q ? q.data() : nullptr, have_q ? q.size() : (size_t)off.back(), nq, block, p)) { printf("invalid\n"); return 0; }
        auto line = [](const char* tag, auto& v) { printf("%s", tag); for (auto x : v) printf(" %llu", (unsigned long long)x); printf("\n"); };
        line("perm", p.perm); line("cell_off", p.cell_off); line("single", p.single); line("entry_of", p.entry_of);
        line("sum_of", p.sum_of); line("entry_at", p.entry_at); line("slot_off", p.slot_off);
        return 0;
    }
    int bad = 0, cases = 0;
    auto run = [&](const char* name, const std::vector<uint64_t>& off, const std::vector<uint32_t>* q, size_t nq, bool want_ok) {
        const size_t m = off.size() - 1;
        for (size_t block : {(size_t)1, (size_t)2, (size_t)3, (size_t)8, (size_t)64, m ? m - 1 : (size_t)5, m ? m : (size_t)1, m + 1, (size_t)1 << 40})
            if (block) { bad += check(name, off, q, nq, block, want_ok); cases++; }
    };
    {   // Groth16-shaped: three shared entries, one private per item; 50 items: a tail block of 2 items at block 8, of 1 item at block 7
        std::vector<uint32_t> q; std::vector<uint64_t> off{0};
        for (uint32_t j = 0; j < 50; j++) { q.insert(q.end(), {3 + j, 0, 1, 2}); off.push_back(q.size()); }
        run("groth16", off, &q, 53, true);
        bad += check("groth16, a tail block of one item", off, &q, 53, 7, true); cases++;
    }
    { std::vector<uint32_t> q{0, 1, 0, 1, 0, 1}; run("kzg: everything shared", {0, 2, 4, 6}, &q, 2, true); }
    run("q_idx NULL", {0, 1, 1, 4, 7}, nullptr, 7, true);
    run("q_idx NULL, nq != np", {0, 3}, nullptr, 4, false);
    { std::vector<uint32_t> q{8, 2, 8, 5, 0, 5, 5, 7}; run("mixed, unreferenced entries, empty items", {0, 0, 3, 3, 8, 8}, &q, 9, true); }
    {   // empty items at the block borders (block 2: items 1, 2 and 3, 4 around them), and blocks with no pairs at all (items 4 to 7)
        std::vector<uint32_t> q{1, 1, 0, 1, 0, 0, 1};
        run("empty items at block borders, blocks with no pairs", {0, 2, 2, 2, 4, 4, 4, 4, 4, 7, 7}, &q, 2, true);
    }
    { std::vector<uint32_t> q{4}; run("one pair", {0, 1}, &q, 5, true); }
    { std::vector<uint32_t> q{4, 4}; run("a single shared entry", {0, 1, 2}, &q, 5, true); }
    { std::vector<uint32_t> q{0, 3}; run("index == nq", {0, 2}, &q, 3, false); }
    { std::vector<uint32_t> q{0}; run("nq = 0 with pairs", {0, 1}, &q, 0, false); }
    { std::vector<uint32_t> q{0, 1}; run("offsets that do not start at 0", {1, 2}, &q, 2, false); }
    { std::vector<uint32_t> q{0, 1, 1}; run("offsets that decrease", {0, 2, 1, 3}, &q, 2, false); }
    { std::vector<uint32_t> q{0, 1, 1}; run("offsets that do not end at np", {0, 2}, &q, 2, false); }
    { std::vector<uint32_t> q; run("np = 0, m = 3", {0, 0, 0, 0}, &q, 4, true); }
    run("np = 0, q_idx NULL", {0, 0}, nullptr, 0, true);
    for (uint32_t seed : {777u, 31337u, 5u}) {                                // pseudo-random indices over a sparse table, ragged items with empty ones
        std::vector<uint32_t> q; std::vector<uint64_t> off{0}; uint32_t x = seed;
        for (int i = 0; i < 3000; i++) {
            x = x * 1664525u + 1013904223u; q.push_back((x >> 9) % (seed == 5u ? 7 : 1200));
            if ((x >> 5) % 3 == 0) off.push_back(q.size());
            if ((x >> 7) % 11 == 0) off.push_back(q.size());
        }
        off.push_back(q.size());
        run("random", off, &q, 1200, true);
    }
    if (bad) return 1;
    printf("PPROD_LOCATE_PLAN ok %d\n", cases);
    return 0;
}
