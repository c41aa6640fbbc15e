// The arithmetic of bls_amd/csrc/fr.h on the host (tests/test_fr_eval_cpu.py compiles this with the address and undefined-behaviour
// sanitizers and runs it directly).  Reads commands on stdin, one a line, and answers each with one or more lines of 64 hex digits:
//   ops A B        A, B: any 256-bit values as 64 hex digits, taken mod r.  One line: mul sqr(A) add sub neg(A) inv(A) A-round-trip, then
//                  is_zero(A) eq(A, B) is_canonical(A) as 0 / 1
//   consts         r, -r^-1 mod 2^32 (as a 256-bit value), R mod r, R^2 mod r, then the 33 entries of the omega_32 table
//   domain k o     the N + 1 entries of domain_table(k, o), out of Montgomery form: the domain in position order, then N^-1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../bls_amd/csrc/fr.h"

using namespace blsmi_fr;

static bool hex32(const char* s, uint8_t out[32]) {
    if (strlen(s) != 64) return false;
    for (int i = 0; i < 32; i++) {
        unsigned v;
        if (sscanf(s + 2 * i, "%2x", &v) != 1) return false;
        out[i] = (uint8_t)v;
    }
    return true;
}
static void put_words(const uint32_t v[8], const char* end) {
    uint8_t be[32];
    store_be32(be, v);
    for (int i = 0; i < 32; i++) printf("%02x", be[i]);
    printf("%s", end);
}
static void put(const Fr& a, const char* end) {
    uint8_t be[32];
    to_be32(a, be);
    for (int i = 0; i < 32; i++) printf("%02x", be[i]);
    printf("%s", end);
}

int main() {
    char cmd[16], sa[80], sb[80];
    while (scanf("%15s", cmd) == 1) {
        if (!strcmp(cmd, "ops")) {
            uint8_t ba[32], bb[32];
            if (scanf("%79s %79s", sa, sb) != 2 || !hex32(sa, ba) || !hex32(sb, bb)) return 2;
            const Fr a = from_be32(ba), b = from_be32(bb);
            uint32_t raw[8];
            load_be32(ba, raw);
            put(mul(a, b), " "); put(sqr(a), " "); put(add(a, b), " "); put(sub(a, b), " "); put(neg(a), " "); put(inv(a), " "); put(a, " ");
            printf("%d %d %d\n", is_zero(a) ? 1 : 0, eq(a, b) ? 1 : 0, is_canonical(raw) ? 1 : 0);
        } else if (!strcmp(cmd, "consts")) {
            const uint32_t m[8] = FR_CONST_MODULUS, ninv[8] = {FR_CONST_NINV, 0, 0, 0, 0, 0, 0, 0}, o[8] = FR_CONST_ONE, r2[8] = FR_CONST_R2;
            static const uint32_t w[33][8] = FR_CONST_OMEGA32;
            put_words(m, "\n"); put_words(ninv, "\n"); put_words(o, "\n"); put_words(r2, "\n");
            for (int i = 0; i < 33; i++) put_words(w[i], "\n");
        } else if (!strcmp(cmd, "domain")) {
            unsigned k; int order;
            if (scanf("%u %d", &k, &order) != 2 || k > MAX_LOG2N || (order != 0 && order != 1)) return 2;
            std::vector<Fr> t(((size_t)1 << k) + 1);
            domain_table(k, order, t.data());
            for (const Fr& e : t) put(e, "\n");
        } else return 2;
    }
    return 0;
}
