// Driver of bls_amd/csrc/group_plan.h for tests/test_rlc_grouped_cpu.py (built with -fsanitize=address,undefined).
// Without arguments: the fixed cases, each checked here (the permutation is a permutation, every group is contiguous and holds exactly the
// tuples of its message in input order, the offsets match the counts, no group is empty); prints "GROUP_PLAN ok <cases>".
// With arguments `d idx0 idx1 ...`: prints the plan of that input (perm / seg_off / msg_of / group_of, one line each) or "range".
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../bls_amd/csrc/group_plan.h"

using blsmi_route::GroupPlan;
using blsmi_route::group_plan;

static int fail(const char* what, const char* name) {
    printf("GROUP_PLAN FAILED %s: %s\n", name, what);
    return 1;
}

static int check(const char* name, const std::vector<uint32_t>& idx, size_t d, bool want_ok) {
    GroupPlan p;
    const size_t n = idx.size();
    const bool ok = group_plan(idx.data(), n, d, p);
    if (ok != want_ok) return fail("verdict", name);
    if (!ok) return 0;
    std::vector<uint64_t> count(d, 0);
    for (uint32_t j : idx) count[j]++;
    size_t nonempty = 0;
    for (uint64_t c : count) nonempty += c != 0;
    if (p.perm.size() != n || p.group_of.size() != n) return fail("sizes", name);
    if (p.msg_of.size() != nonempty || p.seg_off.size() != nonempty + 1) return fail("group count", name);
    if (p.seg_off[0] != 0 || p.seg_off[nonempty] != n) return fail("offsets' ends", name);
    std::vector<uint8_t> seen(n, 0);
    for (uint32_t i : p.perm) {
        if (i >= n || seen[i]) return fail("not a permutation", name);
        seen[i] = 1;
    }
    uint32_t prev_msg = 0;
    for (size_t g = 0; g < nonempty; g++) {
        const uint32_t j = p.msg_of[g];
        if (j >= d || (g && j <= prev_msg)) return fail("msg_of not increasing", name);
        prev_msg = j;
        if (p.seg_off[g + 1] <= p.seg_off[g]) return fail("an empty group", name);
        if (p.seg_off[g + 1] - p.seg_off[g] != count[j]) return fail("offsets do not match the counts", name);
        for (uint64_t k = p.seg_off[g]; k < p.seg_off[g + 1]; k++) {
            const uint32_t i = p.perm[k];
            if (idx[i] != j) return fail("a tuple in another message's group", name);
            if (p.group_of[i] != g) return fail("group_of", name);
            if (k > p.seg_off[g] && p.perm[k - 1] >= i) return fail("input order not kept inside a group", name);
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1) {
        const size_t d = strtoull(argv[1], nullptr, 10);
        std::vector<uint32_t> idx;
        for (int i = 2; i < argc; i++) idx.push_back((uint32_t)strtoul(argv[i], nullptr, 10));
        GroupPlan p;
        if (!group_plan(idx.data(), idx.size(), d, p)) { printf("range\n"); return 0; }
        auto line = [](const char* tag, auto& v) { printf("%s", tag); for (auto x : v) printf(" %llu", (unsigned long long)x); printf("\n"); };
        line("perm", p.perm); line("seg_off", p.seg_off); line("msg_of", p.msg_of); line("group_of", p.group_of);
        return 0;
    }
    int bad = 0, cases = 0;
    auto run = [&](const char* name, const std::vector<uint32_t>& idx, size_t d, bool want_ok) { bad += check(name, idx, d, want_ok); cases++; };
    run("d = 1", std::vector<uint32_t>(7, 0), 1, true);
    { std::vector<uint32_t> v; for (uint32_t i = 0; i < 9; i++) v.push_back(8 - i); run("d = n", v, 9, true); }
    run("empty groups", {5, 2, 5, 5, 9, 2}, 12, true);
    run("an unreferenced first and last entry", {1, 1, 2}, 4, true);
    run("index == d", {0, 3, 1}, 3, false);
    run("index far out of range", {0, 0xffffffffu}, 2, false);
    run("d = 0 with tuples", {0}, 0, false);
    run("n = 0", {}, 5, true);
    run("n = 0, d = 0", {}, 0, true);
    {   // a group of 2^16 + 1 between two small ones, interleaved
        std::vector<uint32_t> v;
        for (uint32_t i = 0; i < (1u << 16) + 1; i++) { v.push_back(1); if (i % 20000 == 0) v.push_back(0); if (i % 30000 == 7) v.push_back(2); }
        run("a group of 2^16 + 1", v, 3, true);
    }
    {   // pseudo-random indices over a sparse table
        std::vector<uint32_t> v; uint32_t x = 12345;
        for (int i = 0; i < 5000; i++) { x = x * 1664525u + 1013904223u; v.push_back((x >> 8) % 97 * 3); }
        run("random", v, 300, true);
    }
    if (bad) return 1;
    printf("GROUP_PLAN ok %d\n", cases);
    return 0;
}
