// Driver of bls_amd/csrc/locate_plan.h for tests/test_rlc_locate_cpu.py (built with -fsanitize=address,undefined).
// Without arguments: the fixed cases, each checked here (the borders run from 0 to n and increase, every block but the last has `block`
// tuples, the record borders are the tuple borders or their halves rounded up, the positions are exactly the tuples of the failing blocks
// in ascending order), and the automatic rule at sampled sizes; prints "LOCATE_PLAN ok <cases>".
// With arguments `n block halved fail0 fail1 ...`: prints the plan (tup_off / rec_off / pos, one line each); block 0 is the automatic rule.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../bls_amd/csrc/locate_plan.h"

using blsmi_route::LocatePlan;
using blsmi_route::locate_auto_block;
using blsmi_route::locate_block_valid;
using blsmi_route::locate_plan;
using blsmi_route::locate_positions;

static int fail(const char* what, const char* name) {
    printf("LOCATE_PLAN FAILED %s: %s\n", name, what);
    return 1;
}

// mode 0: no block fails, 1: all fail, 2: every third block and the last
static int check(const char* name, size_t n, size_t block, bool halved, int mode) {
    LocatePlan p;
    locate_plan(n, block, halved, p);
    const size_t B = p.blocks();
    if (B != (n + block - 1) / block) return fail("block count", name);
    if (p.rec_off.size() != B + 1) return fail("sizes", name);
    if (p.tup_off[0] != 0 || p.rec_off[0] != 0 || p.tup_off[B] != n) return fail("borders' ends", name);
    if (p.rec_off[B] != (halved ? (n + 1) / 2 : n)) return fail("record count", name);
    for (size_t b = 0; b < B; b++) {
        const uint64_t len = p.tup_off[b + 1] - p.tup_off[b];
        if (len == 0 || len > block || (b + 1 < B && len != block)) return fail("block length", name);
        if (p.rec_off[b + 1] != (halved ? (p.tup_off[b + 1] + 1) / 2 : p.tup_off[b + 1])) return fail("record border", name);
        if (p.rec_off[b + 1] <= p.rec_off[b]) return fail("an empty block of records", name);
        if (halved && b + 1 < B && (p.tup_off[b + 1] & 1)) return fail("a border inside a record", name);
    }
    std::vector<uint8_t> f(B ? B : 1, 0);
    for (size_t b = 0; b < B; b++) f[b] = mode == 1 || (mode == 2 && (b % 3 == 0 || b + 1 == B)) ? (uint8_t)(1 + b % 200) : 0;
    std::vector<uint32_t> pos(3, 77);                                      // (stale content must go)
    locate_positions(p, f.data(), pos);
    size_t k = 0;
    for (size_t i = 0; i < n; i++) {
        if (!f[i / block]) continue;
        if (k >= pos.size() || pos[k] != i) return fail("positions", name);
        k++;
    }
    if (k != pos.size()) return fail("positions beyond the failing blocks", name);
    if (mode == 0 && !pos.empty()) return fail("positions although nothing fails", name);
    if (mode == 1 && pos.size() != n) return fail("not every position although everything fails", name);
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 3) {
        const size_t n = strtoull(argv[1], nullptr, 10);
        size_t block = strtoull(argv[2], nullptr, 10);
        const bool halved = atoi(argv[3]) != 0;
        if (!locate_block_valid(block)) { printf("invalid\n"); return 0; }
        if (!block) block = locate_auto_block(n);
        LocatePlan p;
        locate_plan(n, block, halved, p);
        std::vector<uint8_t> f(p.blocks() ? p.blocks() : 1, 0);
        for (int i = 4; i < argc && (size_t)(i - 4) < p.blocks(); i++) f[i - 4] = (uint8_t)atoi(argv[i]);
        std::vector<uint32_t> pos;
        locate_positions(p, f.data(), pos);
        auto line = [](const char* tag, auto& v) { printf("%s", tag); for (auto x : v) printf(" %llu", (unsigned long long)x); printf("\n"); };
        printf("block %llu\n", (unsigned long long)block);
        line("tup_off", p.tup_off); line("rec_off", p.rec_off); line("pos", pos);
        return 0;
    }
    int bad = 0, cases = 0;
    auto run = [&](const char* name, size_t n, size_t block, bool halved) {
        for (int mode = 0; mode < 3; mode++) { bad += check(name, n, block, halved, mode); cases++; }
    };
    run("n = 1", 1, 2, false); run("n = 1, halved", 1, 2, true);
    run("n = block", 8, 8, false); run("n = block, halved", 8, 8, true);
    run("n = block + 1", 9, 8, false); run("n = block + 1, halved", 9, 8, true);
    run("odd n, halved", 71, 8, true); run("odd n", 71, 8, false);
    run("block = 2, halved", 71, 2, true); run("block = 2", 70, 2, false);
    run("block > n", 70, 1024, false); run("block > n, halved", 71, 1024, true);
    run("n = 0", 0, 8, false); run("n = 0, halved", 0, 8, true);
    run("2^16 + 1 in the automatic blocks", 65537, locate_auto_block(65537), true);
    run("2^20 - 1 in blocks of 2", ((size_t)1 << 20) - 1, 2, true);
    // the automatic rule: even, >= 2 (so valid as a caller's value), >= 64, and no more than 257 blocks beyond 16 384 tuples
    size_t sampled = 0;
    for (size_t n = 1; n <= ((size_t)1 << 20); n += n < 70000 ? 1 : 997) {
        const size_t b = locate_auto_block(n);
        if ((b & 1) || b < 2 || b < 64 || !locate_block_valid(b)) { bad += fail("automatic block", "rule"); break; }
        if (b < (n + 255) / 256 || b > std::max<size_t>(64, (n + 255) / 256 + 1)) { bad += fail("automatic block off its formula", "rule"); break; }
        sampled++;
    }
    if (locate_auto_block((size_t)1 << 20) != 4096 || locate_auto_block(65536) != 256 || locate_auto_block(16384) != 64 || locate_auto_block(16640 + 1) != 66) bad += fail("automatic block values", "rule");
    cases++;
    if (locate_block_valid(1) || locate_block_valid(3) || locate_block_valid(71) || !locate_block_valid(0) || !locate_block_valid(2) || !locate_block_valid(1024)) bad += fail("valid blocks", "rule");
    cases++;
    if (bad) return 1;
    printf("LOCATE_PLAN ok %d sampled %llu\n", cases, (unsigned long long)sampled);
    return 0;
}
