// The transform of bls_amd/csrc/fr_ntt.h on the host (tests/test_cell_cpu.py compiles this with the address and undefined-behaviour
// sanitizers and runs it directly).  Reads commands on stdin and answers each with lines of 64 hex digits:
//   interp l o H V_0 .. V_(n-1)    l <= 10, o 0 / 1; H and the n = 2^l values: any 256-bit values as 64 hex digits.  n lines: the coefficients;
//                                  one line: h^n; one line: the flags as a number
//   index l                        for every stage s < l and butterfly t < n / 2 one line `lower partner twiddle`, then bitrev of 0 .. n - 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../bls_amd/csrc/fr_ntt.h"

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
static void put_be(const uint8_t* be) {
    for (int i = 0; i < 32; i++) printf("%02x", be[i]);
    printf("\n");
}

int main() {
    char cmd[16], sv[80];
    while (scanf("%15s", cmd) == 1) {
        if (!strcmp(cmd, "interp")) {
            unsigned l; int order;
            if (scanf("%u %d", &l, &order) != 2 || l > NTT_MAX_LOG2N || (order != 0 && order != 1)) return 2;
            const size_t n = (size_t)1 << l;
            uint8_t h[32], hn[32];
            if (scanf("%79s", sv) != 1 || !hex32(sv, h)) return 2;
            std::vector<uint8_t> vals(32 * n), coeffs(32 * n);                  // exactly the bytes the transform may touch
            for (size_t i = 0; i < n; i++) if (scanf("%79s", sv) != 1 || !hex32(sv, vals.data() + 32 * i)) return 2;
            std::vector<Fr> tab(n + 1);
            domain_table(l, 0, tab.data());
            const unsigned flags = coset_interp(vals.data(), l, order, h, tab.data(), coeffs.data(), hn);
            for (size_t i = 0; i < n; i++) put_be(coeffs.data() + 32 * i);
            put_be(hn);
            printf("%u\n", flags);
            if (coset_interp(vals.data(), l, order, h, tab.data(), coeffs.data(), nullptr) != flags) return 3;   // shift_pow may be null
        } else if (!strcmp(cmd, "index")) {
            unsigned l;
            if (scanf("%u", &l) != 1 || l > NTT_MAX_LOG2N) return 2;
            const uint32_t n = (uint32_t)1 << l;
            for (unsigned s = 0; s < l; s++)
                for (uint32_t t = 0; t < n / 2; t++) { const uint32_t lo = ntt_lower(t, s); printf("%u %u %u\n", lo, ntt_partner(lo, s), ntt_twiddle(t, s, l)); }
            for (uint32_t i = 0; i < n; i++) printf("%u\n", ntt_bitrev(i, l));
        } else return 2;
    }
    return 0;
}
