// Driver of bls_amd/csrc/cell_plan.h (over group_plan.h) for tests/test_rlc_grouped_locate_cpu.py (built with -fsanitize=address,undefined).
// Without arguments: the fixed cases, each checked here (the cells tile perm from 0 to n, none is empty or longer than `block`, none
// crosses a group border, in each group every cell but the last is full, every cell names its group, the positions are exactly the tuples
// of the failing cells with their groups); prints "CELL_PLAN ok <cases>".
// With arguments `d block n idx0 .. idx(n-1) fail0 fail1 ...`: prints the plan (perm / cell_off / group_of / pos / grp, one line each), or
// "invalid" for an index outside the table; block 0 is the automatic rule of locate_plan.h.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../bls_amd/csrc/cell_plan.h"
#include "../../bls_amd/csrc/locate_plan.h"

using blsmi_route::CellPlan;
using blsmi_route::GroupPlan;

static int fail(const char* what, const char* name) {
    printf("CELL_PLAN FAILED %s: %s\n", name, what);
    return 1;
}

// mode 0: no cell fails, 1: all fail, 2: every third cell and the last
static int check(const char* name, const std::vector<uint32_t>& idx, size_t d, size_t block, int mode) {
    const size_t n = idx.size();
    GroupPlan g;
    if (!blsmi_route::group_plan(idx.data(), n, d, g)) return fail("group plan refused", name);
    CellPlan p;
    p.cell_off.assign(5, 9); p.group_of.assign(5, 9);                      // (stale content must go)
    blsmi_route::cell_plan(g, block, p);
    const size_t C = p.cells();
    if (p.group_of.size() != C || p.cell_off[0] != 0 || p.cell_off[C] != n) return fail("sizes / ends", name);
    size_t want = 0;
    for (size_t j = 0; j + 1 < g.seg_off.size(); j++) want += (size_t)((g.seg_off[j + 1] - g.seg_off[j] + block - 1) / block);
    if (C != want) return fail("cell count", name);
    for (size_t c = 0; c < C; c++) {
        const uint64_t lo = p.cell_off[c], hi = p.cell_off[c + 1];
        const uint32_t j = p.group_of[c];
        if (hi <= lo || hi - lo > block) return fail("cell length", name);
        if (j + 1 >= g.seg_off.size() || lo < g.seg_off[j] || hi > g.seg_off[j + 1]) return fail("a cell outside its group", name);
        if (hi != g.seg_off[j + 1] && hi - lo != block) return fail("a short cell that is not its group's last", name);
        if (c && p.group_of[c - 1] > j) return fail("groups out of order", name);
        for (uint64_t k = lo; k < hi; k++) if (g.group_of[g.perm[k]] != j || idx[g.perm[k]] != g.msg_of[j]) return fail("a tuple of another message", name);
    }
    std::vector<uint8_t> f(C ? C : 1, 0);
    for (size_t c = 0; c < C; c++) f[c] = mode == 1 || (mode == 2 && (c % 3 == 0 || c + 1 == C)) ? (uint8_t)(1 + c % 200) : 0;
    std::vector<uint32_t> pos(3, 77), grp(2, 5);
    blsmi_route::cell_positions(g, p, f.data(), pos, grp);
    if (pos.size() != grp.size()) return fail("pos / grp lengths", name);
    size_t k = 0;
    for (size_t c = 0; c < C; c++) {
        if (!f[c]) continue;
        for (uint64_t q = p.cell_off[c]; q < p.cell_off[c + 1]; q++, k++)
            if (k >= pos.size() || pos[k] != g.perm[q] || grp[k] != p.group_of[c] || grp[k] != g.group_of[pos[k]]) return fail("positions", name);
    }
    if (k != pos.size()) return fail("positions beyond the failing cells", name);
    if (mode == 0 && !pos.empty()) return fail("positions although nothing fails", name);
    if (mode == 1 && pos.size() != n) return fail("not every position although everything fails", name);
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 3) {
        const size_t d = strtoull(argv[1], nullptr, 10);
        size_t block = strtoull(argv[2], nullptr, 10);
        const size_t n = strtoull(argv[3], nullptr, 10);
        if ((size_t)argc < 4 + n) return 2;
        std::vector<uint32_t> idx(n);
        for (size_t i = 0; i < n; i++) idx[i] = (uint32_t)strtoul(argv[4 + i], nullptr, 10);
        GroupPlan g;
        if (!blsmi_route::group_plan(idx.data(), n, d, g)) { printf("invalid\n"); return 0; }
        if (!block) block = blsmi_route::locate_auto_block(n);
        CellPlan p;
        blsmi_route::cell_plan(g, block, p);
        std::vector<uint8_t> f(p.cells() ? p.cells() : 1, 0);
        for (size_t i = 4 + n; i < (size_t)argc && i - 4 - n < p.cells(); i++) f[i - 4 - n] = (uint8_t)atoi(argv[i]);
        std::vector<uint32_t> pos, grp;
        blsmi_route::cell_positions(g, p, f.data(), pos, grp);
        auto line = [](const char* tag, auto& v) { printf("%s", tag); for (auto x : v) printf(" %llu", (unsigned long long)x); printf("\n"); };
        printf("block %llu\n", (unsigned long long)block);
        line("perm", g.perm); line("cell_off", p.cell_off); line("group_of", p.group_of); line("pos", pos); line("grp", grp);
        return 0;
    }
    int bad = 0, cases = 0;
    auto run = [&](const char* name, const std::vector<uint32_t>& idx, size_t d, size_t block) {
        for (int mode = 0; mode < 3; mode++) { bad += check(name, idx, d, block, mode); cases++; }
    };
    // the shape of the GPU tests: d = 6 with entry 2 unreferenced, groups of 1, 2, 9, 25, 33, interleaved
    std::vector<uint32_t> base;
    {
        const size_t sizes[6] = {1, 2, 0, 9, 25, 33};
        size_t left[6]; for (int j = 0; j < 6; j++) left[j] = sizes[j];
        for (bool any = true; any;) { any = false; for (int j = 5; j >= 0; j--) if (left[j]) { base.push_back((uint32_t)j); left[j]--; any = true; } }
    }
    run("base, block 4", base, 6, 4); run("base, block 1", base, 6, 1); run("base, block 2", base, 6, 2);
    run("base, block 9 (a group's size)", base, 6, 9); run("base, block 33 (the largest group)", base, 6, 33);
    run("base, block 40 (above every group)", base, 6, 40); run("base, block 1024", base, 6, 1024);
    run("base, block 3 (odd)", base, 6, 3); run("base, a larger table", base, 4096, 4);
    run("one tuple", {0}, 1, 4); run("one tuple, block 1", {3}, 5, 1);
    run("one group", std::vector<uint32_t>(70, 2), 3, 8); run("one group, block = its size", std::vector<uint32_t>(8, 0), 1, 8);
    run("one group, block = its size + 1", std::vector<uint32_t>(8, 0), 1, 9); run("one group, block = its size - 1", std::vector<uint32_t>(8, 0), 1, 7);
    run("n = 0", {}, 4, 8); run("n = 0, d = 0", {}, 0, 8);
    {
        std::vector<uint32_t> all(500);
        for (size_t i = 0; i < 500; i++) all[i] = i < 450 ? 0 : i < 499 ? 2 : 1;
        run("450 / 1 / 49 in cells of 200", all, 3, 200);
        std::vector<uint32_t> big((size_t)1 << 16);
        for (size_t i = 0; i < big.size(); i++) big[i] = (uint32_t)((i * 2654435761u) % 64);
        run("2^16 over 64, the automatic block", big, 64, blsmi_route::locate_auto_block(big.size()));
        run("2^16 over 64, block 1", big, 64, 1);
    }
    {
        GroupPlan g; CellPlan p;
        const uint32_t idx[3] = {0, 5, 1};
        if (blsmi_route::group_plan(idx, 3, 5, g)) bad += fail("an index outside the table accepted", "rule");
        cases++;
    }
    if (bad) return 1;
    printf("CELL_PLAN ok %d\n", cases);
    return 0;
}
