// Driver of bls_amd/csrc/pprod_rlc_plan.h (over group_plan.h) for tests/test_pprod_rlc_cpu.py (built with -fsanitize=address,undefined).
// Without arguments: the fixed cases, each checked here against a direct count (item_of follows the offsets; every group with two or more
// pairs is a shared group holding exactly its entry's pairs in input order, every other one a singleton; the compacted numbering is shared
// first, then singletons, both in table order; group_of agrees with entry_of; split == false leaves no singleton); prints
// "PPROD_RLC_PLAN ok <cases>".  With arguments `nq m off0 .. offm [q0 q1 ...]` (no q: q_idx NULL): prints the plan or "invalid".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../bls_amd/csrc/pprod_rlc_plan.h"

using blsmi_route::PprodRlcPlan;
using blsmi_route::pprod_rlc_plan;

static int fail(const char* what, const char* name) {
    printf("PPROD_RLC_PLAN FAILED %s: %s\n", name, what);
    return 1;
}

static int check(const char* name, const std::vector<uint64_t>& off, const std::vector<uint32_t>* q, size_t nq, bool want_ok, bool split) {
    PprodRlcPlan p;
    const size_t m = off.size() - 1, np = (size_t)off.back() < ((size_t)1 << 24) ? (size_t)off.back() : 0;
    const size_t npairs = q ? q->size() : np;
    static const uint32_t none = 0;                                         // (an empty vector's data() may be null, which would say "no q_idx")
    const bool ok = pprod_rlc_plan(off.data(), m, q ? (q->empty() ? &none : q->data()) : nullptr, npairs, nq, p, split);
    if (ok != want_ok) return fail("verdict", name);
    if (!ok) return 0;
    if (p.item_of.size() != npairs || p.group_of.size() != npairs) return fail("sizes", name);
    for (size_t j = 0; j < m; j++) for (uint64_t k = off[j]; k < off[j + 1]; k++) if (p.item_of[k] != j) return fail("item_of", name);
    std::vector<uint64_t> count(nq, 0);
    for (size_t k = 0; k < npairs; k++) count[q ? (*q)[k] : k]++;
    size_t nsh = 0, nsi = 0;
    for (uint64_t c : count) { if (c >= 2 || (c == 1 && !split)) nsh++; else if (c == 1) nsi++; }
    if (p.shared() != nsh || p.single.size() != nsi || p.groups() != nsh + nsi) return fail("group counts", name);
    if (p.seg_off[0] != 0 || p.seg_off[nsh] != p.perm.size()) return fail("offsets' ends", name);
    std::vector<uint8_t> seen(npairs, 0);
    for (size_t g = 0; g < nsh; g++) {
        const uint32_t e = p.entry_of[g];
        if (e >= nq || (g && e <= p.entry_of[g - 1])) return fail("shared groups not in table order", name);
        if (p.seg_off[g + 1] - p.seg_off[g] != count[e]) return fail("a shared group's size", name);
        for (uint64_t i = p.seg_off[g]; i < p.seg_off[g + 1]; i++) {
            const uint32_t k = p.perm[i];
            if (k >= npairs || seen[k]) return fail("perm repeats or leaves the pairs", name);
            seen[k] = 1;
            if ((q ? (*q)[k] : k) != e || p.group_of[k] != g) return fail("a pair in another entry's group", name);
            if (i > p.seg_off[g] && p.perm[i - 1] >= k) return fail("input order not kept inside a group", name);
        }
    }
    for (size_t t = 0; t < nsi; t++) {
        const uint32_t k = p.single[t], e = p.entry_of[nsh + t];
        if (k >= npairs || seen[k]) return fail("a singleton repeats or leaves the pairs", name);
        seen[k] = 1;
        if (e >= nq || (t && e <= p.entry_of[nsh + t - 1])) return fail("singletons not in table order", name);
        if ((q ? (*q)[k] : k) != e || count[e] != 1 || p.group_of[k] != nsh + t) return fail("a singleton's entry", name);
    }
    for (size_t k = 0; k < npairs; k++) if (!seen[k]) return fail("a pair in no group", name);
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 2) {
        const size_t nq = strtoull(argv[1], nullptr, 10), m = strtoull(argv[2], nullptr, 10);
        if ((size_t)argc < 4 + m) return 2;
        std::vector<uint64_t> off;
        for (size_t i = 0; i <= m; i++) off.push_back(strtoull(argv[3 + i], nullptr, 10));
        std::vector<uint32_t> q;
        for (int i = 4 + (int)m; i < argc; i++) q.push_back((uint32_t)strtoul(argv[i], nullptr, 10));
        const bool have_q = (size_t)argc > 4 + m;
        PprodRlcPlan p;
        if (!pprod_rlc_plan(off.data(), m, have_q ? q.data() : nullptr, have_q ? q.size() : (size_t)off.back(), nq, p)) { printf("invalid\n"); return 0; }
        auto line = [](const char* tag, auto& v) { printf("%s", tag); for (auto x : v) printf(" %llu", (unsigned long long)x); printf("\n"); };
        line("item_of", p.item_of); line("perm", p.perm); line("seg_off", p.seg_off); line("single", p.single); line("entry_of", p.entry_of); line("group_of", p.group_of);
        return 0;
    }
    int bad = 0, cases = 0;
    auto run = [&](const char* name, const std::vector<uint64_t>& off, const std::vector<uint32_t>* q, size_t nq, bool want_ok) {
        bad += check(name, off, q, nq, want_ok, true); bad += check(name, off, q, nq, want_ok, false); cases++;
    };
    {   // Groth16-shaped: three shared entries, one private per item
        std::vector<uint32_t> q; std::vector<uint64_t> off{0};
        for (uint32_t j = 0; j < 50; j++) { q.insert(q.end(), {3 + j, 0, 1, 2}); off.push_back(q.size()); }
        run("groth16", off, &q, 53, true);
    }
    { std::vector<uint32_t> q{0, 1, 0, 1, 0, 1}; run("kzg: everything shared", {0, 2, 4, 6}, &q, 2, true); }
    run("q_idx NULL", {0, 1, 1, 4, 7}, nullptr, 7, true);
    run("q_idx NULL, nq != np", {0, 3}, nullptr, 4, false);
    { std::vector<uint32_t> q{8, 2, 8, 5, 0, 5, 5, 7}; run("mixed, unreferenced entries, empty items", {0, 0, 3, 3, 8, 8}, &q, 9, true); }
    { std::vector<uint32_t> q{4}; run("one pair", {0, 1}, &q, 5, true); }
    { std::vector<uint32_t> q{4, 4}; run("a single shared entry", {0, 1, 2}, &q, 5, true); }
    { std::vector<uint32_t> q{0, 3}; run("index == nq", {0, 2}, &q, 3, false); }
    { std::vector<uint32_t> q{0}; run("nq = 0 with pairs", {0, 1}, &q, 0, false); }
    { std::vector<uint32_t> q{0, 1}; run("offsets that do not start at 0", {1, 2}, &q, 2, false); }
    { std::vector<uint32_t> q{0, 1, 1}; run("offsets that decrease", {0, 2, 1, 3}, &q, 2, false); }
    { std::vector<uint32_t> q{0, 1, 1}; run("offsets that do not end at np", {0, 2}, &q, 2, false); }
    { std::vector<uint32_t> q; run("np = 0, m = 3", {0, 0, 0, 0}, &q, 4, true); }
    run("np = 0, q_idx NULL", {0, 0}, nullptr, 0, true);
    {   // pseudo-random indices over a sparse table, ragged items
        std::vector<uint32_t> q; std::vector<uint64_t> off{0}; uint32_t x = 777;
        for (int i = 0; i < 4000; i++) { x = x * 1664525u + 1013904223u; q.push_back((x >> 9) % 1500); if ((x >> 5) % 3 == 0) off.push_back(q.size()); }
        off.push_back(q.size());
        run("random", off, &q, 1500, true);
    }
    if (bad) return 1;
    printf("PPROD_RLC_PLAN ok %d\n", cases);
    return 0;
}
