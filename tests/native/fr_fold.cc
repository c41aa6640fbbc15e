// The arithmetic of bls_amd/csrc/fr_fold.h on the host (tests/test_groth16_cpu.py compiles this with the address and undefined-behaviour
// sanitizers): one segment of rows folded as k_fr_wsum_u64 / k_fr_wsum_fold fold it.
//   fr_fold [parts] < input        input: "ncol n", then n rows of "weight v_1 .. v_ncol" -- the weight in decimal, the values as 64 hex digits
// Row j goes to partial accumulator j % parts (default 1); the partials meet by halving, as the lanes of a column do, and each of the
// ncol + 1 outputs is reduced once.  Prints the outputs, 64 hex digits a line: the weights' sum first.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../bls_amd/csrc/fr_fold.h"

static bool hex32(const char* s, uint8_t out[32]) {
    if (strlen(s) != 64) return false;
    for (int i = 0; i < 32; i++) {
        unsigned v;
        if (sscanf(s + 2 * i, "%2x", &v) != 1) return false;
        out[i] = (uint8_t)v;
    }
    return true;
}

int main(int argc, char** argv) {
    const size_t parts = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    size_t ncol = 0, n = 0;
    if (parts == 0 || scanf("%zu %zu", &ncol, &n) != 2) { fprintf(stderr, "usage: fr_fold [parts] < input\n"); return 2; }
    const size_t cols = ncol + 1;
    std::vector<blsmi_fr::Acc> acc(parts * cols);
    for (blsmi_fr::Acc& a : acc) blsmi_fr::acc_zero(a);
    std::vector<char> tok(80);
    for (size_t j = 0; j < n; j++) {
        unsigned long long w;
        if (scanf("%llu", &w) != 1) return 2;
        const uint32_t one[8] = {1, 0, 0, 0, 0, 0, 0, 0};
        blsmi_fr::acc_mul_add(acc[(j % parts) * cols], one, w);
        for (size_t i = 0; i < ncol; i++) {
            uint8_t be[32]; uint32_t v[8];
            if (scanf("%79s", tok.data()) != 1 || !hex32(tok.data(), be)) return 2;
            blsmi_fr::load_be32(be, v);
            blsmi_fr::acc_mul_add(acc[(j % parts) * cols + 1 + i], v, w);
        }
    }
    size_t live = parts, h = 1;
    while (h < parts) h <<= 1;
    for (h >>= 1; h >= 1; h >>= 1) {
        for (size_t p = 0; p < h && p + h < live; p++) for (size_t c = 0; c < cols; c++) blsmi_fr::acc_add(acc[p * cols + c], acc[(p + h) * cols + c]);
        if (live > h) live = h;
    }
    for (size_t c = 0; c < cols; c++) {
        uint32_t v[8]; uint8_t be[32];
        blsmi_fr::acc_reduce(acc[c], v);
        blsmi_fr::store_be32(be, v);
        for (int i = 0; i < 32; i++) printf("%02x", be[i]);
        printf("\n");
    }
    return 0;
}
