// fp2_pair.inc -- Fq2 in the LANE-PAIR layout: lanes 2k and 2k+1 of a wave work on the same tuple, the
// even lane holds c0 and the odd lane c1 of every Fq2 element (one Fp per lane).  Partner values are
// fetched with DPP quad_perm [1,0,3,2] (full-rate v_mov_dpp, no LDS).  The per-lane state of a pairing
// halves (f: 90 words), which is what lets two waves share a SIMD without spilling.
// An Fq2 multiplication is ONE fused column pass per lane:
//     even lane  c0 = a0*b0 - a1*b1        odd lane  c1 = a1*b0 + a0*b1
// i.e. mine*P + other*Q with (P,Q) = (b_mine, -b_other) / (b_other, b_mine): 2x225 product MACs + 225
// reduction MACs, a single Montgomery reduction for two products (fq2.go:116-130 needs three).
// Same interface as fp2_single.inc; tower_body.inc / pairing_body.inc compile unchanged on top of it.

template <int L_, int V_> struct Fp2 { static constexpr int L = L_, V = V_; Fp<L_, V_> c; };
template <int L_, int V_> struct Fp6 { static constexpr int L = L_, V = V_; Fp2<L_, V_> c0, c1, c2; };
template <int L_, int V_> struct Fp12 { static constexpr int L = L_, V = V_; Fp6<L_, V_> c0, c1; };
using Fp2S = Fp2<FpS::L, FpS::V>;
using Fp6S = Fp6<FpS::L, FpS::V>;
using Fp12S = Fp12<FpS::L, FpS::V>;
using Fp2R = Fp2<FpR::L, FpR::V>;                    // every coefficient value-reduced (fp.cuh: FpR); Fp*W: what the pairing's values travel in (FpW)
using Fp6R = Fp6<FpR::L, FpR::V>;
using Fp12R = Fp12<FpR::L, FpR::V>;
using Fp2W = Fp2<FpW::L, FpW::V>;
using Fp6W = Fp6<FpW::L, FpW::V>;
using Fp12W = Fp12<FpW::L, FpW::V>;

BLSMI_DEV i32 lane_odd() { return -(i32)(threadIdx.x & 1); }                       // all-ones on odd lanes
BLSMI_DEV i32 bfi(i32 mask, i32 a, i32 b) {                                            // (a & mask) | (b & ~mask) in one VALU op
    i32 r;
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "v"(mask), "v"(a), "v"(b));
    return r;
}
BLSMI_DEV i32 dpp_swap(i32 x) { return __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xf, 0xf, true); }    // quad_perm [1,0,3,2]; every lane has a source lane, so no "old" value is kept (one v_mov_b32_dpp, no copy)
BLSMI_DEV i32 dpp_even(i32 x) { return __builtin_amdgcn_update_dpp(0, x, 0xA0, 0xf, 0xf, true); }    // quad_perm [0,0,2,2]: the pair's even lane (c0) on both lanes
BLSMI_DEV i32 dpp_odd(i32 x) { return __builtin_amdgcn_update_dpp(0, x, 0xF5, 0xf, 0xf, true); }     // quad_perm [1,1,3,3]: the pair's odd lane (c1) on both lanes
template <int L, int V> BLSMI_DEV Fp<L, V> fp_partner(const Fp<L, V>& a) {
    Fp<L, V> r;
#pragma unroll
    for (int i = 0; i < NL; i++) r.v[i] = dpp_swap(a.v[i]);
    return r;
}
template <int L, int V> BLSMI_DEV Fp<L, V> fp_cneg(i32 m, const Fp<L, V>& a) {       // m ? -a : a
    Fp<L, V> r;
#pragma unroll
    for (int i = 0; i < NL; i++) r.v[i] = (a.v[i] ^ m) - m;
    return r;
}
template <int L, int V> BLSMI_DEV Fp2<L, V> wrap(const Fp<L, V>& c) { Fp2<L, V> r; r.c = c; return r; }

template <int L2, int V2, int L, int V>
BLSMI_DEV Fp2<L2, V2> fp2_relabel(const Fp2<L, V>& a) { return wrap(fp_relabel<L2, V2>(a.c)); }
template <int La, int Va, int Lb, int Vb> BLSMI_DEV auto fp2_add(const Fp2<La, Va>& a, const Fp2<Lb, Vb>& b) { return wrap(fp_add(a.c, b.c)); }
template <int La, int Va, int Lb, int Vb> BLSMI_DEV auto fp2_sub(const Fp2<La, Va>& a, const Fp2<Lb, Vb>& b) { return wrap(fp_sub(a.c, b.c)); }
template <int L, int V> BLSMI_DEV auto fp2_neg(const Fp2<L, V>& a) { return wrap(fp_neg(a.c)); }
template <int L, int V> BLSMI_DEV auto fp2_dbl(const Fp2<L, V>& a) { return wrap(fp_dbl(a.c)); }
template <int K, int L, int V> BLSMI_DEV auto fp2_muls(const Fp2<L, V>& a) { return wrap(fp_muls<K>(a.c)); }
template <int L, int V> BLSMI_DEV auto fp2_conj(const Fp2<L, V>& a) { return wrap(fp_cneg(lane_odd(), a.c)); }
template <int L, int V> BLSMI_DEV auto fp2_norm(const Fp2<L, V>& a) { return wrap(fp_norm(a.c)); }
template <int L, int V> BLSMI_DEV Fp2S fp2_store(const Fp2<L, V>& a) { return wrap(fp_store(a.c)); }
template <int L, int V> BLSMI_DEV Fp2R fp2_reduced(const Fp2<L, V>& a) { return wrap(fp_reduced(a.c)); }
template <int L, int V> BLSMI_DEV bool fp2_is_zero(const Fp2<L, V>& a) {
    const int z = fp_is_zero(a.c) ? 1 : 0;
    return (z & __shfl_xor(z, 1)) != 0;
}
template <int La, int Va, int Lb, int Vb> BLSMI_DEV bool fp2_eq(const Fp2<La, Va>& a, const Fp2<Lb, Vb>& b) { return fp2_is_zero(fp2_sub(a, b)); }
template <int L, int V> BLSMI_DEV Fp2<L, V> fp2_select(i32 m, const Fp2<L, V>& a, const Fp2<L, V>& b) { return wrap(fp_select(m, a.c, b.c)); }
BLSMI_DEV Fp2S fp2_zero() { return wrap(fp_zero()); }
BLSMI_DEV Fp2S fp2_one() { return wrap(fp_select(lane_odd(), fp_zero(), fp_one())); }
// constants of consts.cuh are (c0, c1) pairs: each lane keeps its own coefficient
#undef BLSMI_FP2_K
#define BLSMI_FP2_K(x) fp2_pair_const(x)
// a lane-pair Fq2 product costs 907 instructions, a square 714: Fq4 squarings go by two products, not three squares
#undef BLSMI_FP4_SQR_BY_PRODUCTS
#ifndef BLSMI_FP4_SQR_PAIR
#define BLSMI_FP4_SQR_PAIR 1
#endif
#define BLSMI_FP4_SQR_BY_PRODUCTS BLSMI_FP4_SQR_PAIR
BLSMI_DEV Fp2S fp2_pair_const(const blsmi::Fp2S& k) { return wrap(fp_select(lane_odd(), FpS(k.c1), FpS(k.c0))); }

// fq2.go:41-45: (c0 - c1, c0 + c1)
// table of Fq2 values shared by all lanes (entry e = [c0 limbs][c1 limbs]): each lane reads its own coefficient
// (NL_IO = 15 words per coefficient whatever the build; the limbs are this build's own: a table is read by the build that wrote it --
// fp2_table_to_limbs27 turns an entry into the 27-bit kernels' form in place)
BLSMI_DEV Fp2S fp2_table_load(const i32* t, int e) {
    const i32* src = t + (2 * e + (threadIdx.x & 1)) * NL_IO;
    FpS r;
#pragma unroll
    for (int i = 0; i < NL; i++) r.v[i] = src[i];
    return wrap(r);
}
BLSMI_DEV void fp2_table_store(i32* t, int e, const Fp2S& a) {
    i32* dst = t + (2 * e + (threadIdx.x & 1)) * NL_IO;
#pragma unroll
    for (int i = 0; i < NL; i++) dst[i] = a.c.v[i];
}
BLSMI_DEV void fp2_table_to_limbs27(i32* t, int e) {
    i32 w[NL_IO];
    fp_to_limbs27(fp2_table_load(t, e).c, w);
    i32* dst = t + (2 * e + (threadIdx.x & 1)) * NL_IO;
#pragma unroll
    for (int i = 0; i < NL_IO; i++) dst[i] = w[i];
}
template <int L, int V> BLSMI_DEV auto fp2_mul_nr(const Fp2<L, V>& a) { return wrap(fp_add(a.c, fp_cneg(~lane_odd(), fp_partner(a.c)))); }

// (One accumulator per COLUMN -- 27 independent chains, operand-scanning reduction, same 588 multiply-adds -- was measured in round 6 for the lane-row
// kernels at one wave per SIMD: 4 096 pairings 2.25 -> 2.35 ms.  The single chain below is not what bounds a lone wave.)
BLSMI_DEV vlimbs fp2p_mul_body(vlimbs am, vlimbs bm, i32 odd) {
    vlimbs ao, p, q;
    const i32 zero = 0;
#pragma unroll
    for (int i = 0; i < NL; i++) {
        ao[i] = dpp_swap(am[i]);
        p[i] = dpp_even(bm[i]);                           // b0 on both lanes
        q[i] = bfi(odd, bm[i], zero - dpp_swap(bm[i]));   // odd: b1 (mine)   even: -b1
    }
    i32 m[NL];
    vlimbs r;
    i64 acc = 0;
#pragma unroll
    for (int k = 0; k < NL; k++) {
#pragma unroll
        for (int i = 0; i <= k; i++) { acc += (i64)am[i] * p[k - i]; acc += (i64)ao[i] * q[k - i]; }
#pragma unroll
        for (int i = 0; i < k; i++) acc += (i64)m[i] * C_Q[k - i];
        m[k] = (i32)((u32)(i32)acc * BLSMI_QINV) & MASK;
        acc += (i64)m[k] * C_Q[0];
        acc >>= LB;
    }
#pragma unroll
    for (int k = NL; k < 2 * NL - 1; k++) {
#pragma unroll
        for (int i = k - NL + 1; i < NL; i++) { acc += (i64)am[i] * p[k - i]; acc += (i64)ao[i] * q[k - i]; }
#pragma unroll
        for (int i = k - NL + 1; i < NL; i++) acc += (i64)m[i] * C_Q[k - i];
        r[k - NL] = (i32)acc & MASK;
        acc >>= LB;
    }
    r[NL - 1] = (i32)acc;
    return r;
}
#ifdef BLSMI_ASM_CORES
// The cores as assembly blobs behind an inline-asm statement (core_asm.inc, gen_core_asm.py): no function entry, hence no
// s_waitcnt vmcnt(0) that would drain the caller's scratch stores at every product.  a in v[0:15], b in v[16:31]; the product comes back in v[0:15]; the statement names every register the blob writes.
typedef i32 v16i __attribute__((ext_vector_type(16)));
BLSMI_DEV vlimbs fp2p_mul_core(vlimbs a, vlimbs b) BLSMI_CORE_MUL2_STMT(a, b)
#elif defined(BLSMI_PAIR_CORE_INLINE)
BLSMI_DEV vlimbs fp2p_mul_core(vlimbs am, vlimbs bm) { return fp2p_mul_body(am, bm, lane_odd()); }     // (the lane-row unit: A/B switch, see k_pairing_row.hip)
#else
__device__ __noinline__ vlimbs fp2p_mul_core(vlimbs am, vlimbs bm) { return fp2p_mul_body(am, bm, lane_odd()); }
#endif
// fq2.go:75-89: even lane (a0+a1)(a0-a1), odd lane (2*a1)*a0 -- one single-product pass per lane
BLSMI_DEV vlimbs fp2p_sqr_body(vlimbs am, i32 odd) {
    vlimbs x, y;
#pragma unroll
    for (int i = 0; i < NL; i++) {
        const i32 ao = dpp_swap(am[i]);
        x[i] = am[i] + bfi(odd, am[i], ao);          // even: a0 + a1      odd: 2*a1
        y[i] = bfi(odd, ao, am[i] - ao);             // even: a0 - a1      odd: a0
    }
    return fp_mul_body(x, y);
}
#ifdef BLSMI_ASM_CORES
BLSMI_DEV vlimbs fp2p_sqr_core(vlimbs a) BLSMI_CORE_SQR2_STMT(a)
#else
__device__ __noinline__ vlimbs fp2p_sqr_core(vlimbs am) { return fp2p_sqr_body(am, lane_odd()); }
#endif
constexpr int LPROD_MAX2 = LPROD_MAX / 2;            // fused two-product columns: NL*(2*La*Lb+1)*2^(2 LB) < 2^63  (16 for 27-bit limbs, 4 for 28-bit)
template <int La, int Va, int Lb, int Vb>
BLSMI_DEV auto fp2_mul(const Fp2<La, Va>& a, const Fp2<Lb, Vb>& b) {
    if constexpr (La * Lb > LPROD_MAX2) {
        if constexpr (La >= Lb) return fp2_mul(fp2_norm(a), b);
        else return fp2_mul(a, fp2_norm(b));
    } else if constexpr (2LL * Va * Vb > VPROD_MAX) {                    // too large for the fused Montgomery pass: reduce the larger operand (28-bit limbs only)
        if constexpr (Va >= Vb) return fp2_mul(wrap(fp_reduce(a.c)), b); else return fp2_mul(a, wrap(fp_reduce(b.c)));
    } else {
        vlimbs x, y;
#pragma unroll
        for (int i = 0; i < NL; i++) { x[i] = a.c.v[i]; y[i] = b.c.v[i]; }
        const vlimbs z = fp2p_mul_core(x, y);
        Fp2<1, VMUL> r;
#pragma unroll
        for (int i = 0; i < NL; i++) r.c.v[i] = z[i];
        return r;
    }
}
#ifdef BLSMI_PAIR_CORE_INLINE
// where the core is expanded in line (the lane-row unit), fp2_mul_call is the same product through ONE out-of-line copy: for code that would
// otherwise outgrow the instruction cache (the row layout's Miller loops: 29 k instructions with every product expanded)
__device__ __noinline__ vlimbs fp2p_mul_core_out(vlimbs am, vlimbs bm) { return fp2p_mul_body(am, bm, lane_odd()); }
template <int La, int Va, int Lb, int Vb>
BLSMI_DEV auto fp2_mul_call(const Fp2<La, Va>& a, const Fp2<Lb, Vb>& b) {
    if constexpr (La * Lb > LPROD_MAX2) {
        if constexpr (La >= Lb) return fp2_mul_call(fp2_norm(a), b);
        else return fp2_mul_call(a, fp2_norm(b));
    } else if constexpr (2LL * Va * Vb > VPROD_MAX) {
        if constexpr (Va >= Vb) return fp2_mul_call(wrap(fp_reduce(a.c)), b); else return fp2_mul_call(a, wrap(fp_reduce(b.c)));
    } else {
        vlimbs x, y;
#pragma unroll
        for (int i = 0; i < NL; i++) { x[i] = a.c.v[i]; y[i] = b.c.v[i]; }
        const vlimbs z = fp2p_mul_core_out(x, y);
        Fp2<1, VMUL> r;
#pragma unroll
        for (int i = 0; i < NL; i++) r.c.v[i] = z[i];
        return r;
    }
}
#else
template <int La, int Va, int Lb, int Vb> BLSMI_DEV auto fp2_mul_call(const Fp2<La, Va>& a, const Fp2<Lb, Vb>& b) { return fp2_mul(a, b); }
#endif
template <int L, int V>
BLSMI_DEV auto fp2_sqr(const Fp2<L, V>& a) {
    if constexpr (4 * L * L > LPROD_MAX) return fp2_sqr(fp2_norm(a));
    else if constexpr (4LL * V * V > VPROD_MAX) return fp2_sqr(wrap(fp_reduce(a.c)));
    else {
        vlimbs x;
#pragma unroll
        for (int i = 0; i < NL; i++) x[i] = a.c.v[i];
        const vlimbs z = fp2p_sqr_core(x);
        Fp2<1, VMUL> r;
#pragma unroll
        for (int i = 0; i < NL; i++) r.c.v[i] = z[i];
        return r;
    }
}
template <int La, int Va, int Lb, int Vb>
BLSMI_DEV auto fp2_mul_fp(const Fp2<La, Va>& a, const Fp<Lb, Vb>& s) { return wrap(fp_mul(a.c, s)); }
// The Fq inverse of a value BOTH lanes of a pair hold (the norm of fp2_inv): fp_inv_core's safegcd (fp.cuh) with its work split over the two
// lanes, one instruction stream.  The state of the iteration is two independent halves and its transition matrix two independent columns:
//   divsteps     both lanes step (fl, gl, zeta) -- the control masks must agree -- but each carries ONE column of the matrix,
//                the even lane (u, q), the odd lane (v, r); the partner's column arrives by DPP after the batch
//   application  the even lane owns (f, g), the odd lane (d, e); both run the (d, e) form A' = (m0 A + m1 B + mA q) / 2^LB, with the
//                multiple of q forced to zero on even lanes, where the division is exact by construction
// The odd lane reads the low limbs of f and g from the even lane before every batch (LB divsteps look at LB bits: limb 0 holds them all);
// at the end sign(f) comes from the even lane and d from the odd one.  Every limb is computed by the same expression as in
// fp_inv_core, so the result is the same limb for limb: inverse(0) = 0 included (f stays q, d stays 0).
// Per inversion 38.1 k -> 23.4 k executed instructions (33 batches of 1 156 -> 710 as compiled).  -DBLSMI_INV_PAIR_SPLIT=0: both lanes run fp_inv_core
// on the same number (A/B).  Measured, parent and change interleaved five times on one MI355X, 65 536 pairings (profiles/r10_inv_pair_split.log):
// k_final_exp_pair 9.782 -> 9.348 ms (-4.4 %; run-to-run s.d. 0.046), SQ_INSTS_VALU 5.294 G -> 4.963 G wave-instructions per launch (-162 k per
// wave, eleven inversions), k_miller1h_pair 8.31 -> 8.34 ms (unchanged within its spread), the step 18.12 -> 17.72 ms.  DESIGN 3 (v').
#ifndef BLSMI_INV_PAIR_SPLIT
#define BLSMI_INV_PAIR_SPLIT 1
#endif
__device__ __noinline__ vlimbs fp_inv_pair_core(vlimbs a_canon) {
    const i32 odd = lane_odd();
    i32 A[NL], B[NL];                                                      // even lane: (f, g) = (q, a)      odd lane: (d, e) = (0, 1)
#pragma unroll
    for (int i = 0; i < NL; i++) { A[i] = C_Q[i] & ~odd; B[i] = a_canon[i] & ~odd; }
    B[0] |= odd & 1;
    i32 zeta = -1;
    for (int it = 0; it < (878 + LB - 1) / LB + 1; it++) {
        u32 fl = (u32)dpp_even(A[0]), gl = (u32)dpp_even(B[0]);
        u32 t = (u32)(~odd & 1), b = (u32)(odd & 1);                       // my column of the matrix, (top, bottom): (u, q) = (1, 0) or (v, r) = (0, 1)
#pragma unroll
        for (int i = 0; i < LB; i++) {
            u32 c1 = (u32)(zeta >> 31);
            const u32 c2 = 0u - (gl & 1u);
            const u32 x = (fl ^ c1) - c1, y = (t ^ c1) - c1;
            gl += x & c2; b += y & c2;
            c1 &= c2;
            zeta = (i32)((u32)zeta ^ c1) - 1;
            fl += gl & c1; t += b & c1;
            gl >>= 1; t <<= 1;
        }
        const i32 pt = dpp_swap((i32)t), pb = dpp_swap((i32)b);
        const i32 mu = bfi(odd, pt, (i32)t), mv = bfi(odd, (i32)t, pt), mq = bfi(odd, pb, (i32)b), mr = bfi(odd, (i32)b, pb);
        const i32 sa = A[NL - 1] >> 31, sb = B[NL - 1] >> 31;
        i32 ma = (mu & sa) + (mv & sb), mb = (mq & sa) + (mr & sb);
        i64 ca = (i64)mu * A[0] + (i64)mv * B[0], cb = (i64)mq * A[0] + (i64)mr * B[0];
        ma -= (i32)((BLSMI_QINV_POS * (u32)ca + (u32)ma) & (u32)MASK);
        mb -= (i32)((BLSMI_QINV_POS * (u32)cb + (u32)mb) & (u32)MASK);
        ma &= odd; mb &= odd;                                              // (f, g): no multiple of q, the low limb cancels by itself
        ca += (i64)C_Q[0] * ma; cb += (i64)C_Q[0] * mb;
        ca >>= LB; cb >>= LB;
#pragma unroll
        for (int i = 1; i < NL; i++) {
            ca += (i64)mu * A[i] + (i64)mv * B[i] + (i64)C_Q[i] * ma;
            cb += (i64)mq * A[i] + (i64)mr * B[i] + (i64)C_Q[i] * mb;
            A[i - 1] = (i32)ca & MASK; ca >>= LB;
            B[i - 1] = (i32)cb & MASK; cb >>= LB;
        }
        A[NL - 1] = (i32)ca; B[NL - 1] = (i32)cb;
    }
    const i32 sf = dpp_even(A[NL - 1] >> 31);                              // sign(f) * d, as fp_inv_core
    vlimbs out;
#pragma unroll
    for (int i = 0; i < NL; i++) out[i] = (dpp_odd(A[i]) ^ sf) - sf;
    return out;
}
template <int L, int V>
BLSMI_DEV FpS fp_inv_pair(const Fp<L, V>& a) {                             // fp_inv (fp.cuh) around the lane-pair core
    const FpC c = fp_canon(a);
    vlimbs x;
#pragma unroll
    for (int i = 0; i < NL; i++) x[i] = c.v[i];
    const vlimbs z = fp_inv_pair_core(x);
    Fp<2, 3 * VU> r;
#pragma unroll
    for (int i = 0; i < NL; i++) r.v[i] = z[i];
    return fp_store(fp_mul(fp_relabel<1, 3 * VU>(fp_norm(r)), C_R3));
}
// fq2.go:133-147: 1/(c0^2 + c1^2), the same number on both lanes
template <int L, int V>
BLSMI_DEV auto fp2_inv(const Fp2<L, V>& a) {
    const auto n = fp_sqr(a.c);
#if BLSMI_INV_PAIR_SPLIT
    const FpS t = fp_inv_pair(fp_add(n, fp_partner(n)));
#else
    const FpS t = fp_inv(fp_add(n, fp_partner(n)));
#endif
    return wrap(fp_cneg(lane_odd(), fp_mul(a.c, t)));
}
template <int P, int L, int V>
BLSMI_DEV auto fp2_frob(const Fp2<L, V>& a) {
    if constexpr (P % 2 == 0) return a; else return fp2_conj(a);
}
