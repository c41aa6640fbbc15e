// fr_ntt.h -- the index arithmetic and the butterfly of the small inverse transforms in Fr (blsmi 0.22: blsmi_fr_coset_interp_batch*,
// k_fr_ntt.hip), and the interpolation over a coset written out serially.  Plain inline C++ with no HIP types, as fr.h, on which it is
// built: the kernel includes it, and tests/native/fr_ntt.cc runs it natively.
//     a_i = n^-1 sum_k y_k w^(-i k)                    (the inverse DFT of the n = 2^l values y_k = p(h w^k), w the root of fr.h's domains)
//     c_i = h^(-i) a_i                                 (the coefficients of the interpolant I, deg I < n, I = p on the coset h <w>)
// The transform is decimation in time over an array in BIT-REVERSED position order -- position p holds y_bitrev(p) -- and leaves a in natural
// order: stage s = 0 .. l - 1 has n / 2 butterflies t over pairs 2^s apart, within blocks of 2^(s + 1), with the twiddle w^(-(k << (l-1-s))),
// k = t mod 2^s.  Negative powers come from the table of the positive ones: w^(-e) = w^(n - e).
#pragma once
#include "fr.h"

namespace blsmi_fr {

constexpr unsigned NTT_MAX_LOG2N = 10;

// bit reversal over k bits, on either side
FR_FOLD_FN uint32_t ntt_bitrev(uint32_t i, unsigned k) { uint32_t o = 0; for (unsigned b = 0; b < k; b++) o |= ((i >> b) & 1) << (k - 1 - b); return o; }
// butterfly t of stage s: its lower position; the partner is 2^s above it
FR_FOLD_FN uint32_t ntt_lower(uint32_t t, unsigned s) { const uint32_t k = t & (((uint32_t)1 << s) - 1); return ((t - k) << 1) + k; }
FR_FOLD_FN uint32_t ntt_partner(uint32_t lo, unsigned s) { return lo + ((uint32_t)1 << s); }
// ... and the index of its twiddle w^(-(k << (l - 1 - s))) in the order-0 table of the domain of size 2^l (fr.h: domain_table)
FR_FOLD_FN uint32_t ntt_twiddle(uint32_t t, unsigned s, unsigned l) {
    const uint32_t n = (uint32_t)1 << l, e = (t & (((uint32_t)1 << s) - 1)) << (l - 1 - s);
    return (n - e) & (n - 1);
}
// (a, b) <- (a + w b, a - w b)
FR_FOLD_FN void ntt_butterfly(Fr& a, Fr& b, const Fr& w) { const Fr t = mul(b, w); b = sub(a, t); a = add(a, t); }
// g^i for i below 2^l, with g^0 = 1 whatever g: l squarings, a product per set bit
FR_FOLD_FN Fr ntt_pow_small(const Fr& g, uint32_t i, unsigned l) {
    Fr acc = one(), p = g;
    for (unsigned b = 0; b < l; b++) {
        if ((i >> b) & 1) acc = mul(acc, p);
        p = sqr(p);
    }
    return acc;
}
// g^(2^l)
FR_FOLD_FN Fr ntt_pow_pow2(const Fr& g, unsigned l) { Fr p = g; for (unsigned b = 0; b < l; b++) p = sqr(p); return p; }
// the 256-bit value v (little-endian words, ANY value) as the Montgomery form of v / n: ONE product by n^-1 R^2, made of the table's n^-1 R
FR_FOLD_FN Fr ntt_scale_factor(const Fr& ninv) { return from_words(ninv.w); }
FR_FOLD_FN Fr ntt_load_scaled(const uint32_t v[8], const Fr& factor) { Fr o; mont_mul_words(factor.w, v, o.w); return o; }

// The interpolation of one item, serially (host only).  vals: n = 2^l values of 32 big-endian bytes, ANY value taken mod r; order 0: position
// i is the value at h w^i, order 1: at h w^bitrev(i); shift: h, 32 big-endian bytes, taken mod r; tab: the order-0 domain table of size n
// (n + 1 elements).  coeffs: n fully reduced scalars, the coefficient of X^i at i; shift_pow: h^n mod r (may be null); returns the flags:
// bit 0: a value or the shift was >= r, bit 1: h = 0 mod r -- then h^-1 counts as 0 and 0^0 as 1: c_0 = a_0, every other c_i = 0.
inline unsigned coset_interp(const uint8_t* vals, unsigned l, int order, const uint8_t* shift, const Fr* tab, uint8_t* coeffs, uint8_t* shift_pow) {
    const uint32_t n = (uint32_t)1 << l;
    const Fr factor = ntt_scale_factor(tab[n]);
    Fr* a = new Fr[n];
    unsigned flags = 0;
    for (uint32_t i = 0; i < n; i++) {
        uint32_t v[8];
        load_be32(vals + 32 * (size_t)i, v);
        if (!is_canonical(v)) flags |= 1;
        a[order ? i : ntt_bitrev(i, l)] = ntt_load_scaled(v, factor);
    }
    for (unsigned s = 0; s < l; s++)
        for (uint32_t t = 0; t < n / 2; t++) {
            const uint32_t lo = ntt_lower(t, s);
            ntt_butterfly(a[lo], a[ntt_partner(lo, s)], tab[ntt_twiddle(t, s, l)]);
        }
    uint32_t hw[8];
    load_be32(shift, hw);
    if (!is_canonical(hw)) flags |= 1;
    const Fr h = from_words(hw), hinv = inv(h);
    if (is_zero(h)) flags |= 2;
    for (uint32_t i = 0; i < n; i++) to_be32(mul(a[i], ntt_pow_small(hinv, i, l)), coeffs + 32 * (size_t)i);
    if (shift_pow) to_be32(ntt_pow_pow2(h, l), shift_pow);
    delete[] a;
    return flags;
}

}  // namespace blsmi_fr
