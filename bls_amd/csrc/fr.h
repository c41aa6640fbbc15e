// fr.h -- the scalar field Fr of BLS12-381 proper (blsmi 0.21: blsmi_fr_mul_batch*, blsmi_fr_inv_batch*, blsmi_fr_eval_batch*,
// k_fr_eval.hip): Montgomery product and inversion mod r, and the evaluation domains.  Plain inline C++ with no HIP types, as fr_fold.h,
// whose qualifier FR_FOLD_FN and whose byte order helpers it uses: the kernels include it, and tests/native/fr_field.cc runs it natively.
//     r = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001,        R = 2^256 (the Montgomery radix)
// An element is eight 32-bit words, little-endian, the Montgomery form x R mod r of x, ALWAYS below r: equality is word equality.  The
// 32 x 32 + 64 multiply-add is the one of fr_fold.h.  r < 2^255, so a sum of two elements fits eight words and one conditional subtraction
// restores the bound after a sum or a product.  The constants are fr_consts.h, generated with big integers by gen_fr_consts.py.
#pragma once
#include "fr_fold.h"
#include "fr_consts.h"

namespace blsmi_fr {

struct Fr { uint32_t w[8]; };

// d = v - r; returns the borrow: 1 exactly when v < r
FR_FOLD_FN uint32_t sub_modulus(const uint32_t v[8], uint32_t d[8]) {
    const uint32_t M[8] = FR_CONST_MODULUS;
    uint64_t borrow = 0;
    for (int i = 0; i < 8; i++) { const uint64_t t = (uint64_t)v[i] - M[i] - borrow; d[i] = (uint32_t)t; borrow = (t >> 32) & 1; }
    return (uint32_t)borrow;
}
// v below 2 r to v mod r
FR_FOLD_FN void reduce_once(uint32_t v[8]) {
    uint32_t d[8];
    const uint32_t keep = sub_modulus(v, d);
    for (int i = 0; i < 8; i++) v[i] = keep ? v[i] : d[i];
}
// is the 256-bit value v a canonical scalar (below r)?
FR_FOLD_FN bool is_canonical(const uint32_t v[8]) { uint32_t d[8]; return sub_modulus(v, d) != 0; }
// v mod r for ANY 256-bit v: 2^256 - 1 < 3 r, two conditional subtractions
FR_FOLD_FN void reduce_any(uint32_t v[8]) { reduce_once(v); reduce_once(v); }

// out = a b / R mod r, fully reduced, for a b < r R -- one factor below r, the other ANY 256-bit value.  Word by word (CIOS): row i adds
// a b_i, then the multiple m r of the modulus that clears the lowest word, and shifts one word down; the running value stays below 2 r
// < 2^256, so the ninth word is zero after every shift and t[9] never carries.
FR_FOLD_FN void mont_mul_words(const uint32_t a[8], const uint32_t b[8], uint32_t out[8]) {
    const uint32_t M[8] = FR_CONST_MODULUS;
    uint32_t t[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 8; i++) {
        uint64_t c = 0;
        for (int j = 0; j < 8; j++) { const uint64_t s = (uint64_t)a[j] * b[i] + t[j] + c; t[j] = (uint32_t)s; c = s >> 32; }
        uint64_t s = (uint64_t)t[8] + c; t[8] = (uint32_t)s; t[9] = (uint32_t)(s >> 32);
        const uint32_t m = t[0] * FR_CONST_NINV;
        s = (uint64_t)m * M[0] + t[0]; c = s >> 32;
        for (int j = 1; j < 8; j++) { s = (uint64_t)m * M[j] + t[j] + c; t[j - 1] = (uint32_t)s; c = s >> 32; }
        s = (uint64_t)t[8] + c; t[7] = (uint32_t)s; t[8] = t[9] + (uint32_t)(s >> 32);
    }
    for (int i = 0; i < 8; i++) out[i] = t[i];
    reduce_once(out);
}

FR_FOLD_FN Fr zero() { Fr o; for (int i = 0; i < 8; i++) o.w[i] = 0; return o; }
FR_FOLD_FN Fr one() { const uint32_t v[8] = FR_CONST_ONE; Fr o; for (int i = 0; i < 8; i++) o.w[i] = v[i]; return o; }
FR_FOLD_FN bool is_zero(const Fr& a) { uint32_t o = 0; for (int i = 0; i < 8; i++) o |= a.w[i]; return o == 0; }
FR_FOLD_FN bool eq(const Fr& a, const Fr& b) { uint32_t o = 0; for (int i = 0; i < 8; i++) o |= a.w[i] ^ b.w[i]; return o == 0; }

FR_FOLD_FN Fr mul(const Fr& a, const Fr& b) { Fr o; mont_mul_words(a.w, b.w, o.w); return o; }
FR_FOLD_FN Fr sqr(const Fr& a) { return mul(a, a); }
FR_FOLD_FN Fr add(const Fr& a, const Fr& b) {
    Fr o; uint64_t c = 0;
    for (int i = 0; i < 8; i++) { const uint64_t t = (uint64_t)a.w[i] + b.w[i] + c; o.w[i] = (uint32_t)t; c = t >> 32; }   // (below 2^256: no carry out)
    reduce_once(o.w);
    return o;
}
FR_FOLD_FN Fr sub(const Fr& a, const Fr& b) {
    const uint32_t M[8] = FR_CONST_MODULUS;
    Fr o; uint64_t borrow = 0, c = 0;
    for (int i = 0; i < 8; i++) { const uint64_t t = (uint64_t)a.w[i] - b.w[i] - borrow; o.w[i] = (uint32_t)t; borrow = (t >> 32) & 1; }
    const uint32_t mask = (uint32_t)0 - (uint32_t)borrow;                        // a < b: add r back
    for (int i = 0; i < 8; i++) { const uint64_t t = (uint64_t)o.w[i] + (M[i] & mask) + c; o.w[i] = (uint32_t)t; c = t >> 32; }
    return o;
}
FR_FOLD_FN Fr neg(const Fr& a) { return sub(zero(), a); }

// ANY 256-bit value, little-endian words, taken mod r, to Montgomery form: v R^2 / R -- the product reduces (v R^2 < 2^256 r)
FR_FOLD_FN Fr from_words(const uint32_t v[8]) { const uint32_t r2[8] = FR_CONST_R2; Fr o; mont_mul_words(v, r2, o.w); return o; }
// back: the fully reduced value, little-endian words
FR_FOLD_FN void to_words(const Fr& a, uint32_t v[8]) { const uint32_t u[8] = {1, 0, 0, 0, 0, 0, 0, 0}; mont_mul_words(a.w, u, v); }
// the same over 32 big-endian bytes (the library's scalars)
FR_FOLD_FN Fr from_be32(const uint8_t* p) { uint32_t v[8]; load_be32(p, v); return from_words(v); }
FR_FOLD_FN void to_be32(const Fr& a, uint8_t* p) { uint32_t v[8]; to_words(a, v); store_be32(p, v); }

// a^-1, and 0 for 0: Fermat's a^(r - 2), square and multiply from the top bit (254) down.  One inversion per polynomial is what an
// evaluation pays (k_fr_inv), so nothing cleverer is here.
FR_FOLD_FN Fr inv(const Fr& a) {
    const uint32_t e[8] = FR_CONST_EXP_INV;
    Fr x = a;                                                                    // bit 254 of r - 2 is set
    for (int b = 253; b >= 0; b--) {
        x = sqr(x);
        if ((e[b >> 5] >> (b & 31)) & 1) x = mul(x, a);
    }
    return x;
}

// ---- the evaluation domains (host only) --------------------------------------------------------------------------------------------------
// The domain of size N = 2^k, k <= 16: the N-th roots of unity w^0 .. w^(N-1), w = 7^((r - 1) / N).  order 0: position i holds w^i;
// order 1: position i holds w^bitrev_k(i) (the layout of an EIP-4844 blob).
constexpr unsigned MAX_LOG2N = 16;
inline uint32_t bitrev(uint32_t i, unsigned k) { uint32_t o = 0; for (unsigned b = 0; b < k; b++) o |= ((i >> b) & 1) << (k - 1 - b); return o; }
// w for the domain of size 2^k (k <= 32), in Montgomery form
inline Fr domain_root(unsigned k) {
    static const uint32_t W[33][8] = FR_CONST_OMEGA32;
    return from_words(W[32 - k]);
}
// out[0 .. N-1]: the domain in POSITION order, Montgomery form; out[N]: N^-1 -- the table the kernels read (N + 1 elements)
inline void domain_table(unsigned k, int order, Fr* out) {
    const size_t n = (size_t)1 << k;
    const Fr w = domain_root(k);
    Fr p = one();
    for (size_t e = 0; e < n; e++) { out[order ? bitrev((uint32_t)e, k) : e] = p; p = mul(p, w); }   // (bit reversal is its own inverse)
    const uint32_t nn[8] = {(uint32_t)n, 0, 0, 0, 0, 0, 0, 0};
    out[n] = inv(from_words(nn));
}

}  // namespace blsmi_fr
