// mul_u64.cuh -- the 64-bit ladder of the randomised batch verifications, for the units that run it: k_curve.hip (k_g?_mul_u64,
// k_g?_segsum_chunk_u64, one lane per point) and k_msm_pair.hip (k_g2_segsum_chunk_u64_pair, F = the lane-pair Fq2).  Include after curve.cuh.
#pragma once
// 64-bit scalars (the randomised batch verification, verify_host.inc: rlc_shard): the fixed 4-bit window of mul_batch_body over 16 nibbles --
// 60 doublings and 15 additions after the 14 of the table, uniform control flow for all 64 lanes.  A plain ladder, not the endomorphisms:
// the hash points of the cofactor-power route and a caller's keys need not lie in the subgroup, and the product is exact for any curve point.
// Infinity is not special-cased: the caller flags it (zero records).
template <class F>
BLSMI_DEV Jac<F> mul_u64_jac(const Aff<F>& p, u64 k) {
    Jac<F> tab[16];
    tab[0] = jac_zero<F>();
    tab[1] = to_jac(p);
    for (int j = 2; j < 16; j++) tab[j] = jac_add_affine(tab[j - 1], p);
    Jac<F> res = tab[(u32)(k >> 60)];
    for (int nib = 14; nib >= 0; nib--) {
        res = jac_double(res); res = jac_double(res); res = jac_double(res); res = jac_double(res);
        res = jac_add(res, tab[(u32)(k >> (4 * nib)) & 15]);
    }
    return res;
}
