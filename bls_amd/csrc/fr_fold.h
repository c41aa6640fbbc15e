// fr_fold.h -- arithmetic of the weighted folds in the scalar field Fr (blsmi 0.19: blsmi_fr_wsum_segmented_u64*, k_fr.hip): a wide integer
// accumulator for sums of 64 x 256-bit products, its carry-resolving addition, and the one reduction mod r an output gets.  Plain inline
// C++ with no HIP types: the kernels include it, and tests/native/fr_fold.cc runs it natively (FR_FOLD_FN is empty there).
//     r = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001        (the order of G1, G2 and GT of BLS12-381)
// An accumulator is twelve 32-bit words, little-endian: 2^32 rows x (2^64 - 1) x (2^256 - 1) stays below 2^352 <= 2^384, so no sum of a
// call (n <= 2^32 - 1 rows) overflows, whatever the values -- nothing is reduced per row.
#pragma once
#include <cstddef>
#include <cstdint>

#ifndef FR_FOLD_FN
#ifdef __HIPCC__
#define FR_FOLD_FN __host__ __device__ inline
#else
#define FR_FOLD_FN inline
#endif
#endif

namespace blsmi_fr {

constexpr int ACC_WORDS = 12;
struct Acc { uint32_t w[ACC_WORDS]; };

FR_FOLD_FN void acc_zero(Acc& a) { for (int i = 0; i < ACC_WORDS; i++) a.w[i] = 0; }

// the 32-byte big-endian scalar at p as eight little-endian words, and back
FR_FOLD_FN void load_be32(const uint8_t* p, uint32_t v[8]) {
    for (int k = 0; k < 8; k++) { const uint8_t* q = p + 28 - 4 * k; v[k] = (uint32_t)q[0] << 24 | (uint32_t)q[1] << 16 | (uint32_t)q[2] << 8 | q[3]; }
}
FR_FOLD_FN void store_be32(uint8_t* p, const uint32_t v[8]) {
    for (int k = 0; k < 8; k++) { uint8_t* q = p + 28 - 4 * k; q[0] = (uint8_t)(v[k] >> 24); q[1] = (uint8_t)(v[k] >> 16); q[2] = (uint8_t)(v[k] >> 8); q[3] = (uint8_t)v[k]; }
}

// a += wt * v: two rows of eight 32 x 32 products, each row's carry run to the top word.  (A row's step is at most
// (2^32 - 1)^2 + 2 (2^32 - 1) = 2^64 - 1: the 64-bit intermediate never overflows.)
FR_FOLD_FN void acc_mul_add(Acc& a, const uint32_t v[8], uint64_t wt) {
    const uint32_t wl[2] = {(uint32_t)wt, (uint32_t)(wt >> 32)};
    for (int h = 0; h < 2; h++) {
        uint64_t c = 0;
        for (int i = 0; i < 8; i++) { const uint64_t t = (uint64_t)v[i] * wl[h] + a.w[i + h] + c; a.w[i + h] = (uint32_t)t; c = t >> 32; }
        for (int i = 8 + h; i < ACC_WORDS; i++) { const uint64_t t = (uint64_t)a.w[i] + c; a.w[i] = (uint32_t)t; c = t >> 32; }
    }
}
// a += b, the carries resolved word by word
FR_FOLD_FN void acc_add(Acc& a, const Acc& b) {
    uint64_t c = 0;
    for (int i = 0; i < ACC_WORDS; i++) { const uint64_t t = (uint64_t)a.w[i] + b.w[i] + c; a.w[i] = (uint32_t)t; c = t >> 32; }
}

// a mod r, fully reduced, as eight little-endian words.  Binary long division from the highest nonzero word down: the remainder stays
// below r < 2^255, so twice it plus a bit fits eight words and one subtraction restores the bound.  One call per output, never per row.
FR_FOLD_FN void acc_reduce(const Acc& a, uint32_t out[8]) {
    const uint32_t R[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};
    uint32_t rem[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int top = ACC_WORDS - 1;
    while (top > 0 && a.w[top] == 0) top--;
    for (int wi = top; wi >= 0; wi--) {
        const uint32_t word = a.w[wi];
        for (int b = 31; b >= 0; b--) {
            uint32_t in = (word >> b) & 1;
            for (int i = 0; i < 8; i++) { const uint32_t o = rem[i] >> 31; rem[i] = rem[i] << 1 | in; in = o; }
            uint32_t d[8]; uint64_t borrow = 0;                               // d = rem - r; kept when it does not borrow
            for (int i = 0; i < 8; i++) { const uint64_t t = (uint64_t)rem[i] - R[i] - borrow; d[i] = (uint32_t)t; borrow = (t >> 32) & 1; }
            if (!borrow) for (int i = 0; i < 8; i++) rem[i] = d[i];
        }
    }
    for (int i = 0; i < 8; i++) out[i] = rem[i];
}

}  // namespace blsmi_fr
