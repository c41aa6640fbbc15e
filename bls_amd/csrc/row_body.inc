// row_body.inc -- the pairing in the LANE-ROW layout: SIXTEEN adjacent lanes (one DPP row) per tuple.  Included inside namespace
// blsmi::pairl after tower_body.inc / pairing_body.inc, on top of the unchanged lane-pair Fq2 layer (fp2_pair.inc: the even lane of a
// pair holds c0, the odd lane c1 of an Fq2).
//
// Why (VERDICT r05 item 1): the reference's API produces calls of a few thousand tuples at most (one tuple per Verify, 128-signer
// aggregates: g2pubs/bls.go:159-162, g1pubs/verify_benchmark_test.go:33-85).  4 096 tuples are 256 waves in the lane-quad layout -- a
// quarter of the chip's 1 024 SIMDs -- and 4 096 waves on the one-tuple-per-wave path, whose level programs spend 30.5 M
// lane-instructions on a pairing.  Here 4 096 tuples are 1 024 waves, one per SIMD, and a lane carries a twelfth of an Fq12.
//
// Layout.  Fq12 = Fq2[w] / (w^6 - xi) (w^2 = v, v^3 = xi): the eight lane pairs of a row are numbered p = 0 .. 7 and pair p holds the
// coefficient of w^p -- in the reference's names (fq12.go:9-13, fq6.go:9-14) c_h.c_j with h = p & 1, j = p >> 1 -- for p < 6; pairs 6
// and 7 carry nothing (they run along: one instruction stream).  So
//   * a DPP quad (lanes 4j .. 4j+3) holds (c0.c_j, c1.c_j): the two Fq6 halves meet through quad_perm [2,3,0,1], one v_mov_dpp per limb;
//   * the three coefficients of an Fq6 half sit in quads 0, 1, 2 at the same position: they rotate through row_ror:4 / 8 / 12 with a
//     bank mask (two v_mov_dpp per limb);
//   * the Fq4 = Fq2[w^3] pairs of a cyclotomic squaring are (p, p + 3): row_ror:6 / 10.
// Every lane pair runs ONE instruction stream -- an Fq2 product (fp2p_mul_core, the lane-pair kernels' core) or a fused sum of three
// (fp2p_mul3_core below) -- on its own operands: an Fq12 product is three product times (lane pair: 18, lane quad: 9), an Fq12
// squaring two (12 / 6), a sparse line multiplication ONE fused pass (13 / 8), a Granger-Scott squaring one (6 / 3), a doubling step
// with its line evaluated at P two (9 + 2 scalings / 5 + 1).  What each pair feeds into the stream is a per-lane v_bfi select; no LDS.
// Same field elements as the lane-pair routines: the Miller value is the homogeneous steps' of pairing_body.inc, the final
// exponentiation the same chain (pairing.go:79-129) with plain Granger-Scott squarings (a compressed run saves nothing when the
// three Fq4 squarings already run side by side).

// The Fq12 routines are functions of their own -- a value is 14 registers, in and out by value -- with their product cores expanded inside them
// (k_pairing_row.hip: BLSMI_PAIR_CORE_INLINE); the Miller loops' step functions are expanded into the loops and call ONE out-of-line copy of the core
// (fp2_mul_call).  -DBLSMI_ROW_INLINE expands the routines into their callers as well: measured, slower (k_miller2_row 1.66 -> 1.81 ms: 235 KB of code).
#ifdef BLSMI_ROW_INLINE
#define BLSMI_RFN BLSMI_DEV
#else
#define BLSMI_RFN BLSMI_NOINLINE
#endif

BLSMI_DEV int row_pair() { return (threadIdx.x >> 1) & 7; }
// all-ones on the lanes of the pairs whose bit is set in M
template <unsigned M> BLSMI_DEV i32 pm() { return (i32)((u32)M << (31 - row_pair())) >> 31; }
constexpr unsigned RQ0 = 0x03, RQ1 = 0x0C, RQ2 = 0x30, REVEN = 0x55, RODD = 0xAA;     // quads 0 .. 2; the pairs of half c0 / half c1
template <int CTRL, int BANK> BLSMI_DEV i32 dpp_row(i32 old, i32 x) { return __builtin_amdgcn_update_dpp(old, x, CTRL, 0xf, BANK, BANK == 0xf); }

// ---- moving values between the pairs of a row (profiles/r06_dpp_probe.txt: row_ror:n gives lane i the value of lane i - n mod 16) ----
// rrot<K>: pair p receives pair p - K (mod 8)
template <int K, int L, int V> BLSMI_DEV Fp2<L, V> rrot(const Fp2<L, V>& a) {
    constexpr int k = ((K % 8) + 8) % 8;
    if constexpr (k == 0) return a;
    else {
        Fp2<L, V> r;
#pragma unroll
        for (int i = 0; i < NL; i++) r.c.v[i] = dpp_row<0x120 + 2 * k, 0xf>(0, a.c.v[i]);
        return r;
    }
}
// qswap: the other pair of the same quad (the other Fq6 half's coefficient of the same v-power)
template <int L, int V> BLSMI_DEV Fp2<L, V> qswap(const Fp2<L, V>& a) {
    Fp2<L, V> r;
#pragma unroll
    for (int i = 0; i < NL; i++) r.c.v[i] = dpp_row<0x4E, 0xf>(0, a.c.v[i]);
    return r;
}
// qrot<D>: quad j receives quad j + D mod 3 (j = 0, 1, 2; quad 3 receives something): the coefficients of an Fq6 half rotate
template <int D, int L, int V> BLSMI_DEV Fp2<L, V> qrot(const Fp2<L, V>& a) {
    static_assert(D == 1 || D == 2, "rotation among three quads");
    Fp2<L, V> r;
#pragma unroll
    for (int i = 0; i < NL; i++) {
        if constexpr (D == 1) r.c.v[i] = dpp_row<0x128, 0x4>(dpp_row<0x12C, 0xf>(0, a.c.v[i]), a.c.v[i]);     // quads 0, 1 <- the next quad; quad 2 <- quad 0
        else r.c.v[i] = dpp_row<0x128, 0x1>(dpp_row<0x124, 0xf>(0, a.c.v[i]), a.c.v[i]);                      // quads 1, 2 <- the previous quad; quad 0 <- quad 2
    }
    return r;
}
// bcast<P>: every pair receives pair P's value (row_newbcast of its even and of its odd lane)
template <int P, int L, int V> BLSMI_DEV Fp2<L, V> bcast(const Fp2<L, V>& a) {
    const i32 odd = lane_odd();
    Fp2<L, V> r;
#pragma unroll
    for (int i = 0; i < NL; i++) r.c.v[i] = bfi(odd, dpp_row<0x150 + 2 * P + 1, 0xf>(0, a.c.v[i]), dpp_row<0x150 + 2 * P, 0xf>(0, a.c.v[i]));
    return r;
}
// rsel<M>: a on the pairs of M, b elsewhere
template <unsigned M, int La, int Va, int Lb, int Vb>
BLSMI_DEV auto rsel(const Fp2<La, Va>& a, const Fp2<Lb, Vb>& b) {
    constexpr int L = imax(La, Lb), V = imax(Va, Vb);
    return fp2_select(pm<M>(), fp2_relabel<L, V>(a), fp2_relabel<L, V>(b));
}
// the row layout's storage form: limbs normalised, |value| < 2.01 q (a stored value enters sums of up to six before a product)
using Fp2R = Fp2<1, VRED>;
template <int L, int V> BLSMI_DEV Fp2R fp2_tight(const Fp2<L, V>& a) {
    if constexpr (V <= VRED) return fp2_relabel<1, VRED>(fp2_norm(a));
    else return wrap(fp_reduce(a.c));
}

// ---- three Fq2 products summed in ONE Montgomery pass: a1 b1 + a2 b2 + a3 b3 (operands with normalised limbs).  Per column six product
// multiply-adds and one reduction multiply-add instead of 3 x (2 + 1): 1 372 against 1 764 multiply-adds, no recombination.
BLSMI_DEV vlimbs fp2p_mul3_body(vlimbs a1, vlimbs b1, vlimbs a2, vlimbs b2, vlimbs a3, vlimbs b3, i32 odd) {
    static_assert((double)NL * 7.0 * 1.01 < (double)(1ull << (63 - 2 * LB)), "six products and the reduction term overflow the 64-bit column");
    vlimbs o1, p1, q1, o2, p2, q2, o3, p3, q3;
    const i32 zero = 0;
#pragma unroll
    for (int i = 0; i < NL; i++) {
        o1[i] = dpp_swap(a1[i]); p1[i] = dpp_even(b1[i]); q1[i] = bfi(odd, b1[i], zero - dpp_swap(b1[i]));
        o2[i] = dpp_swap(a2[i]); p2[i] = dpp_even(b2[i]); q2[i] = bfi(odd, b2[i], zero - dpp_swap(b2[i]));
        o3[i] = dpp_swap(a3[i]); p3[i] = dpp_even(b3[i]); q3[i] = bfi(odd, b3[i], zero - dpp_swap(b3[i]));
    }
    i32 m[NL];
    vlimbs r;
    i64 acc = 0;
#pragma unroll
    for (int k = 0; k < NL; k++) {
#pragma unroll
        for (int i = 0; i <= k; i++) {
            acc += (i64)a1[i] * p1[k - i]; acc += (i64)o1[i] * q1[k - i];
            acc += (i64)a2[i] * p2[k - i]; acc += (i64)o2[i] * q2[k - i];
            acc += (i64)a3[i] * p3[k - i]; acc += (i64)o3[i] * q3[k - i];
        }
#pragma unroll
        for (int i = 0; i < k; i++) acc += (i64)m[i] * C_Q[k - i];
        m[k] = (i32)((u32)(i32)acc * BLSMI_QINV) & MASK;
        acc += (i64)m[k] * C_Q[0];
        acc >>= LB;
    }
#pragma unroll
    for (int k = NL; k < 2 * NL - 1; k++) {
#pragma unroll
        for (int i = k - NL + 1; i < NL; i++) {
            acc += (i64)a1[i] * p1[k - i]; acc += (i64)o1[i] * q1[k - i];
            acc += (i64)a2[i] * p2[k - i]; acc += (i64)o2[i] * q2[k - i];
            acc += (i64)a3[i] * p3[k - i]; acc += (i64)o3[i] * q3[k - i];
        }
#pragma unroll
        for (int i = k - NL + 1; i < NL; i++) acc += (i64)m[i] * C_Q[k - i];
        r[k - NL] = (i32)acc & MASK;
        acc >>= LB;
    }
    r[NL - 1] = (i32)acc;
    return r;
}
// (expanded in line at its few call sites: as a function its 84 argument registers and ~200 live ones run into the callee-saved half of the
// register file -- 129 scratch accesses per call in the first build)
BLSMI_DEV vlimbs fp2p_mul3_core(vlimbs a1, vlimbs b1, vlimbs a2, vlimbs b2, vlimbs a3, vlimbs b3) { return fp2p_mul3_body(a1, b1, a2, b2, a3, b3, lane_odd()); }
template <int V1, int W1, int V2, int W2, int V3, int W3>
BLSMI_DEV Fp2<1, VMUL> fp2_mul3(const Fp2<1, V1>& a1, const Fp2<1, W1>& b1, const Fp2<1, V2>& a2, const Fp2<1, W2>& b2, const Fp2<1, V3>& a3, const Fp2<1, W3>& b3) {
    static_assert(2LL * ((long long)V1 * W1 + (long long)V2 * W2 + (long long)V3 * W3) <= VPROD_MAX, "the fused sum leaves the Montgomery pass's range: reduce an operand");
    vlimbs x1, y1, x2, y2, x3, y3;
#pragma unroll
    for (int i = 0; i < NL; i++) { x1[i] = a1.c.v[i]; y1[i] = b1.c.v[i]; x2[i] = a2.c.v[i]; y2[i] = b2.c.v[i]; x3[i] = a3.c.v[i]; y3[i] = b3.c.v[i]; }
    const vlimbs z = fp2p_mul3_core(x1, y1, x2, y2, x3, y3);
    Fp2<1, VMUL> r;
#pragma unroll
    for (int i = 0; i < NL; i++) r.c.v[i] = z[i];
    return r;
}

// ---- an Fq12 value of one tuple: pair p (< 6) holds the coefficient of w^p ------------------------------------------------------------
struct R12 { Fp2R c; };
BLSMI_DEV R12 r12_one() {
    const Fp2S s = rsel<0x01>(fp2_one(), fp2_zero());
    R12 r;
#pragma unroll
    for (int i = 0; i < NL; i++) r.c.c.v[i] = s.c.v[i];                                // (0 and 1 in canonical form: inside the tight bound)
    return r;
}
BLSMI_DEV void r12_conj_inplace(R12& a) { a.c = wrap(fp_cneg(pm<RODD>(), a.c.c)); }                      // fq12.go:27-29: c1 = -c1 (the odd powers of w)
// from / to the lane-pair form of the same value (every pair of the row holds all of it there)
BLSMI_DEV R12 r12_from_pair(const Fp12S& f) {
    R12 r;
    r.c = fp2_tight(rsel<0x01>(f.c0.c0, rsel<0x02>(f.c1.c0, rsel<0x04>(f.c0.c1, rsel<0x08>(f.c1.c1, rsel<0x10>(f.c0.c2, rsel<0x20>(f.c1.c2, fp2_zero())))))));
    return r;
}
BLSMI_DEV Fp12S r12_to_pair(const R12& a) {
    Fp12S r;
    r.c0.c0 = fp2_store(bcast<0>(a.c)); r.c1.c0 = fp2_store(bcast<1>(a.c)); r.c0.c1 = fp2_store(bcast<2>(a.c));
    r.c1.c1 = fp2_store(bcast<3>(a.c)); r.c0.c2 = fp2_store(bcast<4>(a.c)); r.c1.c2 = fp2_store(bcast<5>(a.c));
    return r;
}
BLSMI_DEV bool r12_is_one(const R12& a) {
    int e = fp2_eq(a.c, rsel<0x01>(fp2_one(), fp2_zero())) ? 1 : 0;
    e |= row_pair() >= 6 ? 1 : 0;
    e &= __shfl_xor(e, 2); e &= __shfl_xor(e, 4); e &= __shfl_xor(e, 8);
    return e != 0;
}

// ---- Fq6 products by Karatsuba (fq6.go:255-292), BOTH halves of the row at once: the coefficient U_j of an operand sits in quad j (on the
// even pair for one product, on the odd pair for another).  Round 1 multiplies the plain products P_j = U_j V_j, round 2 the sums'
//   quad 0: (U1 + U2)(V1 + V2)      quad 1: (U0 + U1)(V0 + V1)      quad 2: (U0 + U2)(V0 + V2)
// -- each quad gets the sum product ITS output coefficient needs -- and k6_recombine puts c_j together in quad j.
template <int L, int V> BLSMI_DEV auto k6_sumop(const Fp2<L, V>& u) {
    const auto u1 = qrot<1>(u), u2 = qrot<2>(u);                                       // quad j: U_(j+1), U_(j+2)
    return fp2_add(rsel<RQ0>(u1, u), rsel<RQ2>(u1, u2));                              // U1 + U2 | U1 + U0 | U2 + U0
}
template <int L, int V> BLSMI_DEV auto k6_mulv(const Fp2<L, V>& u) {                    // fq6.go:34-37: times v = (xi U2, U0, U1)
    const auto t = qrot<2>(u);
    return rsel<RQ0>(fp2_mul_nr(t), t);
}
//   c0 = P0 + xi (S0 - P1 - P2)      c1 = S1 - P0 - P1 + xi P2      c2 = S2 - P0 - P2 + P1
template <int Lp, int Vp, int Ls, int Vs> BLSMI_DEV auto k6_recombine(const Fp2<Lp, Vp>& p, const Fp2<Ls, Vs>& s) {
    const auto p1 = qrot<1>(p), p2 = qrot<2>(p);                                       // quad 0: P1, P2    quad 1: P2, P0    quad 2: P0, P1
    // (limbs stay un-normalised through here: 3 + 3 + 1 times the normalised bound at the end, inside the head-room; the callers normalise once)
    const auto e = fp2_sub(fp2_sub(s, rsel<RQ0>(p1, p)), rsel<RQ2>(p1, p2));            // S - P1 - P2 | S - P1 - P0 | S - P0 - P2
    const auto xg = fp2_mul_nr(rsel<RQ0>(e, p1));                                      // xi e | xi P2
    return rsel<RQ0>(fp2_add(xg, p), rsel<RQ1>(fp2_add(e, xg), fp2_add(e, p2)));
}

// fq12.go:180-195.  ab = a0 a1 on the even pairs, t = (a0 + v a1)(a0 + a1) on the odd pairs -- two Fq6 products in two product times --;
// c0 = t - ab - v ab, c1 = 2 ab
BLSMI_RFN R12 r12_sqr(const R12 a) {
    const auto o = qswap(a.c);                                                         // the other half's coefficient of the same quad
    const auto u = fp2_norm(rsel<REVEN>(a.c, fp2_add(o, k6_mulv(a.c))));               // even: a0_j    odd: a0_j + (v a1)_j
    const auto v = fp2_norm(rsel<REVEN>(o, fp2_add(a.c, o)));                          // even: a1_j    odd: a0_j + a1_j
    const auto p = fp2_norm(fp2_mul(u, v));
    const auto s = fp2_norm(fp2_mul(k6_sumop(u), k6_sumop(v)));
    const auto R = fp2_norm(k6_recombine(p, s));                                       // even: ab_j    odd: t_j
    const auto Ro = qswap(R);
    R12 r;
    r.c = fp2_tight(rsel<REVEN>(fp2_sub(fp2_sub(Ro, R), k6_mulv(R)), fp2_add(Ro, Ro)));
    return r;
}
// fq12.go:198-213, Karatsuba over the halves and inside them: c0 = a0 b0 + v a1 b1, c1 = (a0 + a1)(b0 + b1) - a0 b0 - a1 b1.  Rounds 1 and 2
// multiply a0 b0 (even pairs) and a1 b1 (odd pairs); round 3 the third Fq6 product, its plain products on the even pairs and its sum
// products on the odd pairs, where c1 lives: three product times.
BLSMI_RFN R12 r12_mul(const R12 a, const R12 b) {
    const auto as = fp2_norm(k6_sumop(a.c)), bs = fp2_norm(k6_sumop(b.c));
    const auto p = fp2_norm(fp2_mul(a.c, b.c));
    const auto s = fp2_norm(fp2_mul(as, bs));
    const auto R = fp2_norm(k6_recombine(p, s));                                       // even: (a0 b0)_j    odd: (a1 b1)_j
    const auto x = fp2_add(a.c, qswap(a.c)), y = fp2_add(b.c, qswap(b.c));            // (a0 + a1)_j, (b0 + b1)_j on both pairs of quad j
    const auto xs = fp2_add(as, qswap(as)), ys = fp2_add(bs, qswap(bs));              // their sum operands (k6_sumop is linear)
    const auto q = fp2_norm(fp2_mul(rsel<REVEN>(x, xs), rsel<REVEN>(y, ys)));         // even: plain products    odd: sum products
    const auto T = fp2_norm(k6_recombine(qswap(q), q));                               // odd pairs: ((a0 + a1)(b0 + b1))_j
    const auto Ro = qswap(R);
    R12 r;
    r.c = fp2_tight(rsel<REVEN>(fp2_add(R, k6_mulv(Ro)), fp2_sub(fp2_sub(T, Ro), R)));
    return r;
}
// fq12.go:32-47: a (c0 + c1 v + c4 v w) = a (c0 + c1 w^2 + c4 w^3), the line's coefficients on every pair:
//   out_k = a_k c0 + xi^[k < 2] a_(k-2) c1 + xi^[k < 3] a_(k-3) c4      (indices mod 6) -- one fused pass
template <int V0, int V1, int V4>
BLSMI_DEV R12 r12_mul_by_014_i(const R12& a, const Fp2<1, V0>& c0, const Fp2<1, V1>& c1, const Fp2<1, V4>& c4) {
    const auto a2 = fp2_norm(rsel<0x03>(fp2_mul_nr(rrot<4>(a.c)), rrot<2>(a.c)));      // pairs 0, 1 <- xi a_4, xi a_5; pair k <- a_(k-2)
    const auto a3 = fp2_norm(rsel<0x07>(fp2_mul_nr(rrot<5>(a.c)), rrot<3>(a.c)));      // pairs 0 .. 2 <- xi a_3 .. xi a_5; pair k <- a_(k-3)
    R12 r;
    r.c = fp2_tight(fp2_mul3(a.c, c0, a2, c1, a3, c4));
    return r;
}
BLSMI_NOINLINE R12 r12_mul_by_014(const R12 a, const Fp2R c0, const Fp2R c1, const Fp2R c4) { return r12_mul_by_014_i(a, c0, c1, c4); }   // (the unit tests' entry; the loops expand _i in line)

// Granger-Scott squaring on the cyclotomic subgroup (tower_body.inc: fp12_cyclotomic_sqr).  In Fq4 = Fq2[s], s = w^3, the value is
// A + B w + C w^2 with A = (z0, z1) on pairs (0, 3), B = (z2, z3) on (1, 4), C = (z4, z5) on (2, 5); its square is
// (3 A^2 - 2 conj A) + (3 s C^2 + 2 conj B) w + (3 B^2 - 2 conj C) w^2.  The three Fq4 squarings (p + q s)^2 = (t - v - xi v) + 2 v s,
// t = (p + q)(p + xi q), v = p q run side by side: pairs 0 .. 2 multiply t, pairs 3 .. 5 multiply v -- ONE product time (lane quad: 3).
BLSMI_RFN R12 r12_cyc_sqr(const R12 f) {
    const auto& z = f.c;
    const auto o = rsel<0x07>(rrot<5>(z), rrot<3>(z));                                 // the Fq4 partner: pairs 0 .. 2 get q, pairs 3 .. 5 get p
    const auto xo = fp2_mul_nr(o);
    const auto P = fp2_norm(fp2_mul(rsel<0x07>(fp2_add(z, o), o), rsel<0x07>(fp2_add(z, xo), z)));   // pairs 0 .. 2: t of A, B, C    pairs 3 .. 5: v
    const auto vo = rrot<5>(P);                                                        // pairs 0 .. 2: v of A, B, C
    const auto xvo = fp2_mul_nr(vo);
    const auto W = rsel<0x07>(fp2_sub(fp2_sub(P, vo), xvo), fp2_dbl(P));     // pairs 0 .. 2: A^2, B^2, C^2 `first`    pairs 3 .. 5: `second`
    // where the squares go: A^2 stays (pairs 0, 3); B^2 moves to C's pairs (2, 5 <- 1, 4); s C^2 = xi second + first s to B's (pair 4 <- first
    // of pair 2, pair 1 <- xi second = 2 xi v, which pair 2 holds as 2 xvo)
    const auto D = fp2_norm(rsel<0x09>(W, rsel<0x24>(rrot<1>(W), rsel<0x10>(rrot<2>(W), fp2_dbl(rrot<7>(xvo))))));   // (the one normalisation: 3 D + 2 z below)
    // 3 D -+ 2 z: minus on the even powers of w (conj of an Fq4 negates its s-coefficient, which sits on pairs 3, 4, 5 = w^3, w^4, w^5;
    // with the sign of the formulas above: z0, z4, z3 -> minus on pairs 0, 2, 4; z1, z2, z5 -> plus on pairs 3, 1, 5)
    const auto zs = wrap(fp_cneg(pm<REVEN>(), z.c));
    R12 r;
    r.c = fp2_tight(fp2_add(fp2_dbl(fp2_add(D, zs)), D));
    return r;
}

// ---- Miller loop (pairing.go:16-75) with the homogeneous steps of pairing_body.inc: doubling_step_h_i's formulas
//   A = XY, B = Y^2, E = 12 xi Z^2, H = 2YZ, F = 3E, G = B + F;   X3 = 2 A (B - F), Y3 = G^2 - 12 E^2, Z3 = 4 B H;   line (B - E) + (-3 X^2) xP v + H yP v w
// The running point is held by EVERY pair (45 words a lane).  Round 1: pairs 0 .. 5 multiply XY, YZ, Y^2, X^2, Z^2, YZ; round 2: A (B - F), (YZ) B,
// G^2, X^2 xP, E^2, (YZ) yP -- the line's two scalings by P's coordinates ride along as Fq2 products with (xP, 0), (yP, 0).
// The line evaluated at P, on every pair: c0 a stored value, c1 and c4 fresh products -- all normalised, none reduced: the fused line product has the
// head-room (2 (5 * 22 + 10 * 3 + 10 * 3) of 4 096).
struct RLine { Fp2S c0; Fp2<1, VMUL> c1, c4; };
// P's coordinates as the Fq2 constants the steps multiply by -- (-3 xP, 0) for the doubling's line (-3 X^2) xP, (-xP, 0) for the addition's (-th) xP,
// (yP, 0) -- kept PACKED in one register set (even lane: -xP, odd lane: yP; 14 registers instead of 42) and unpacked where a step needs them: the Miller
// loops live at the edge of the 256-register budget, and what does not fit goes to scratch (DESIGN 7: a round trip costs thousands of cycles)
BLSMI_DEV Fp2S r_scalar(const FpS& s) { return wrap(fp_select(lane_odd(), fp_zero(), s)); }   // (s, 0) as an Fq2
struct RPoint {
    FpS v;
    BLSMI_DEV Fp2S PXa() const { return r_scalar(v); }
    BLSMI_DEV auto PXd() const { return fp2_muls<3>(r_scalar(v)); }
    BLSMI_DEV Fp2S PY() const { return r_scalar(fp_partner(v)); }
};
BLSMI_DEV RPoint r_point(const FpS& px, const FpS& py) { RPoint p; p.v = fp_select(lane_odd(), py, fp_store(fp_neg(px))); return p; }
// a G2 point's affine record in memory: the addition steps (five a loop) read it again instead of holding 28 registers for it through the loop
struct RQ {
    const u8* rec; int par;
    BLSMI_DEV void load(Fp2S& x, Fp2S& y) const { x = wrap(load_be48(rec + 48 * par)); y = wrap(load_be48(rec + 96 + 48 * par)); }
};
// A prepared line (the generator's table, pairing_body.inc: load_line) waiting for its two scalings by the OTHER pair's P: they ride along in the
// last round of the running point's step, on pairs that round leaves idle -- no product time of their own.  xy: even lane xP', odd lane yP'
struct RQval { Fp2S x, y; BLSMI_DEV void load(Fp2S& a, Fp2S& b) const { a = x; b = y; } };      // (the unit test's: a point held in registers)
struct RTab {
    Fp2S o0, o1, o2; FpS xy;
    BLSMI_DEV Fp2S PX() const { return r_scalar(xy); }
    BLSMI_DEV Fp2S PY() const { return r_scalar(fp_partner(xy)); }
};
template <int L, int V> BLSMI_DEV Fp2S r_stored(const Fp2<L, V>& a) { static_assert(L == 1 && V <= FpS::V, "already a storable value"); return fp2_relabel<FpS::L, FpS::V>(a); }
// Small factors ride on OPERANDS (a product's operand may carry limbs up to 4 x the normalised bound): H = Y (2Z), X3 = A (2 (B - F)), Z3 = H (4B),
// Y3 = G^2 - 3 (E (4E)), the line's -3 in (-3 xP, 0) -- so the products come out as the values wanted, normalised.  E = 12 xi Z^2 is reduced once
// (72 -> 2 q): everything built from it then multiplies without a further reduction.
template <bool TAB>
BLSMI_DEV void r_doubling_step(G2Proj& r, const RPoint& P, RLine& l, const RTab* t = nullptr, RLine* lt = nullptr) {
    // pair 0: X Y = A    1: Y 2Z = H    2: Y Y = B    3: X X    4: Z Z    5: Y 2Z = H
    const auto P1 = fp2_norm(fp2_mul_call(rsel<0x09>(r.x, rsel<0x10>(r.z, r.y)), rsel<0x05>(r.y, rsel<0x08>(r.x, rsel<0x10>(r.z, fp2_dbl(r.z))))));
    const auto B = bcast<2>(P1), Z2 = bcast<4>(P1);
    const auto E = fp2_tight(fp2_muls<12>(fp2_norm(fp2_mul_nr(Z2))));
    const auto F = fp2_muls<3>(E);
    const auto G = fp2_norm(fp2_add(B, F));
    const auto y2 = rsel<0x01>(fp2_dbl(fp2_norm(fp2_sub(B, F))), rsel<0x02>(fp2_muls<4>(B), rsel<0x04>(G, rsel<0x08>(P.PXd(), rsel<0x10>(fp2_muls<4>(E), P.PY())))));
    // pair 0: A 2(B - F) = X3    1: H 4B = Z3    2: G^2    3: X^2 (-3 xP) = c1    4: E 4E    5: H yP = c4    [6: o1 xP', 7: o0 yP' of the prepared line]
    Fp2<1, VMUL> P2;
    if constexpr (TAB) P2 = fp2_norm(fp2_mul_call(rsel<0x04>(G, rsel<0x10>(E, rsel<0x40>(t->o1, rsel<0x80>(t->o0, P1)))), rsel<0x40>(t->PX(), rsel<0x80>(t->PY(), y2))));
    else P2 = fp2_norm(fp2_mul_call(rsel<0x04>(G, rsel<0x10>(E, P1)), y2));
    l.c0 = fp2_store(fp2_sub(B, E));
    l.c1 = bcast<3>(P2); l.c4 = bcast<5>(P2);
    if constexpr (TAB) { lt->c0 = t->o2; lt->c1 = bcast<6>(P2); lt->c4 = bcast<7>(P2); }
    r.x = r_stored(bcast<0>(P2)); r.z = r_stored(bcast<1>(P2));
    r.y = fp2_store(bcast<2>(fp2_sub(P2, fp2_muls<3>(rrot<6>(P2)))));                  // pair 2: G^2 - 12 E^2
}
// the mixed addition R + Q and its chord (pairing_body.inc: addition_step_h), four product times instead of eleven + two scalings:
//   th = Y - yq Z, la = X - xq Z;  C = th^2, D = la^2;  E = la D, F = Z C, G = X D;  Hh = E + F - 2G;  X3 = la Hh, Y3 = th (G - Hh) - E Y, Z3 = Z E
//   line (th xq - la yq) + (-th) xP v + la yP v w
template <bool TAB, class QSRC>
BLSMI_DEV void r_addition_step(G2Proj& r, const QSRC& q, const RPoint& P, RLine& l, const RTab* t = nullptr, RLine* lt = nullptr) {
    Fp2S qx, qy;
    q.load(qx, qy);
    const auto P1 = fp2_norm(fp2_mul_call(rsel<0x01>(qy, qx), r.z));                        // pair 0: yq Z    pair 1: xq Z
    const auto th = fp2_norm(fp2_sub(r.y, bcast<0>(P1))), la = fp2_norm(fp2_sub(r.x, bcast<1>(P1)));
    // pair 0: th^2    1: la^2    2: th xq    3: la yq    4: th (-xP) = c1    5: la yP = c4    6: la^2
    const auto P2 = fp2_norm(fp2_mul_call(rsel<0x15>(th, la), rsel<0x01>(th, rsel<0x42>(la, rsel<0x04>(qx, rsel<0x08>(qy, rsel<0x10>(P.PXa(), P.PY())))))));
    const auto P3 = fp2_norm(fp2_mul_call(rsel<0x01>(r.z, rsel<0x02>(la, r.x)), P2));       // pair 0: Z C = F    1: la D = E    6: X D = G
    const auto F = bcast<0>(P3), E = bcast<1>(P3), G = bcast<6>(P3);
    const auto Hh = fp2_norm(fp2_sub(fp2_add(E, F), fp2_dbl(G)));
    const auto y4 = rsel<0x01>(Hh, rsel<0x02>(fp2_norm(fp2_sub(G, Hh)), rsel<0x04>(r.y, r.z)));
    // pair 0: la Hh    1: th (G - Hh)    2: E Y    3: Z E    [4: o1 xP', 5: o0 yP' of the prepared line]
    Fp2<1, VMUL> P4;
    if constexpr (TAB) P4 = fp2_norm(fp2_mul_call(rsel<0x01>(la, rsel<0x02>(th, rsel<0x10>(t->o1, rsel<0x20>(t->o0, E)))), rsel<0x10>(t->PX(), rsel<0x20>(t->PY(), y4))));
    else P4 = fp2_norm(fp2_mul_call(rsel<0x01>(la, rsel<0x02>(th, E)), y4));
    // (differences of two pairs' products are taken AFTER the broadcasts: `P - rrot<7>(P)` makes the compiler fold the move into v_subrev_u32_dpp,
    // which computes the un-reversed difference on gfx950 -- tools/dpp_sub_probe.hip, tests/test_isa_guards.py)
    l.c0 = fp2_store(fp2_sub(bcast<2>(P2), bcast<3>(P2)));                              // th xq - la yq
    l.c1 = bcast<4>(P2); l.c4 = bcast<5>(P2);
    if constexpr (TAB) { lt->c0 = t->o2; lt->c1 = bcast<4>(P4); lt->c4 = bcast<5>(P4); }
    r.x = r_stored(bcast<0>(P4)); r.y = fp2_store(fp2_sub(bcast<1>(P4), bcast<2>(P4))); r.z = r_stored(bcast<3>(P4));
}
// The three loops below each write out their walk over the bits of |x| >> 1, in one shape: a bit is a loop over its steps -- the doubling, then the
// addition where |x|'s bit is set -- that ends in ONE expansion site of the fused line product (it is expanded in line; code size: -DBLSMI_ROW_INLINE
// above shows what 235 KB of code cost), then the squaring.  That shape is not pairing_body.inc's x_bit_walk, which has two sites a bit.  A walker of
// this shape shared by the three loops (a template over the step, the steps a closure or a step object) was built and measured: the same
// multiply-adds, but the compiler lays the blocks out otherwise and copies a line (41 moves) at the loop head -- k_miller1h_row 0.976 -> 1.003 ms per
// 4 096 (the parent's worst of five runs: 0.989), the 2 304-signer aggregates 2.863 -> 2.908 and 3.995 -> 4.036 ms (profiles/r14_pairing_bodies.log).
// These kernels are instruction-count bound at the edge of their register budget, so the loops stay written out.
// one (P, Q) pair: the value k_miller1h_pair computes
BLSMI_DEV void miller_loop_r(R12& f, const FpS& px, const FpS& py, const RQ& q) {
    G2Proj r; q.load(r.x, r.y); r.z = fp2_one();
    const RPoint P = r_point(px, py);
    f = r12_one();
    const u64 xr = BLSMI_X_ABS >> 1;
    RLine l;
    // ONE site of the fused line multiplication (it is expanded in line): steps = the doubling, then the addition where |x|'s bit is set
    for (int i = 61; i >= -1; i--) {
        const int steps = (i >= 0 && ((xr >> i) & 1)) ? 2 : 1;
        for (int st = 0; st < steps; st++) {
            if (st == 0) r_doubling_step<false>(r, P, l); else r_addition_step<false>(r, q, P, l);
            f = r12_mul_by_014_i(f, l.c0, l.c1, l.c4);
        }
        if (i >= 0) f = r12_sqr(f);
    }
    r12_conj_inplace(f);                                                               // blsIsNegative (pairing.go:71-73)
}
// two (P, Q) pairs sharing the squarings (CompareTwoPairings, pairing.go:140-147; the verify family): the step's two lines go into f one after
// the other -- two fused passes (the lane-pair kernels multiply the lines together first: 6 + 17 products; here that would be 1 + 3 product times
// against 2 fused passes).  PRE0: pair 0's G2 point is the generator, its 68 line triples are read from `pre`; their scalings by P0's coordinates
// ride along in point 1's steps (RTab).
template <bool PRE0>
BLSMI_DEV void miller_loop2_r(R12& f, const FpS (&px)[2], const FpS (&py)[2], const RQ (&q)[2], const i32* pre) {
    G2Proj r0, r1;
    if (!PRE0) { q[0].load(r0.x, r0.y); r0.z = fp2_one(); }
    q[1].load(r1.x, r1.y); r1.z = fp2_one();
    const RPoint P0 = r_point(px[0], py[0]), P1 = r_point(px[1], py[1]);
    f = r12_one();
    const u64 xr = BLSMI_X_ABS >> 1;
    RLine l, lt;
    int line = 0;
    for (int i = 61; i >= -1; i--) {
        const int steps = (i >= 0 && ((xr >> i) & 1)) ? 2 : 1;
        if constexpr (PRE0) {
            RTab t; t.xy = fp_select(lane_odd(), py[0], px[0]);
            for (int st = 0; st < steps; st++) {
                load_line(pre, line++, t.o0, t.o1, t.o2);
                if (st == 0) r_doubling_step<true>(r1, P1, l, &t, &lt); else r_addition_step<true>(r1, q[1], P1, l, &t, &lt);
                for (int k = 0; k < 2; k++) {                                          // (one expansion of the fused line product for both lines: code size)
                    const RLine& c = k ? l : lt;
                    f = r12_mul_by_014_i(f, c.c0, c.c1, c.c4);
                }
            }
        } else {
            for (int st = 0; st < 2 * steps; st++) {                                   // doubling of point 0, of point 1, then (bit set) the two additions
                if (st == 0) r_doubling_step<false>(r0, P0, l);
                else if (st == 1) r_doubling_step<false>(r1, P1, l);
                else if (st == 2) r_addition_step<false>(r0, q[0], P0, l);
                else r_addition_step<false>(r1, q[1], P1, l);
                f = r12_mul_by_014_i(f, l.c0, l.c1, l.c4);
            }
        }
        if (i >= 0) f = r12_sqr(f);
    }
    r12_conj_inplace(f);
}

// One pair whose G2 point is the GENERATOR: no running point, the 68 prepared lines are read from `pre` and scaled by P's coordinates (one
// product time a line: pair 0 multiplies o1 (xP, 0), pair 1 multiplies o0 (yP, 0)).  The signature side of a g2pubs Verify (e(sig, G2One),
// g2pubs/bls.go:161), run on a side stream while the message is hashed.
BLSMI_DEV void miller_loop_table_r(R12& f, const FpS& px, const FpS& py, const i32* pre) {
    const Fp2S PX = r_scalar(px), PY = r_scalar(py);
    f = r12_one();
    const u64 xr = BLSMI_X_ABS >> 1;
    int line = 0;
    for (int i = 61; i >= -1; i--) {
        const int steps = (i >= 0 && ((xr >> i) & 1)) ? 2 : 1;
        for (int st = 0; st < steps; st++) {
            Fp2S o0, o1, o2;
            load_line(pre, line++, o0, o1, o2);
            const auto sc = fp2_norm(fp2_mul_call(rsel<0x01>(o1, o0), rsel<0x01>(PX, PY)));
            f = r12_mul_by_014_i(f, o2, bcast<0>(sc), bcast<1>(sc));
        }
        if (i >= 0) f = r12_sqr(f);
    }
    r12_conj_inplace(f);
}

// ---- final exponentiation (pairing.go:79-129), the chain of pairing_body.inc over R12 -----------------------------------------------
// fq12.go:216-237: 1 / a = conj(a) / (a conj(a)); a conj(a) = a0^2 - v a1^2 lies in Fq6 (the even pairs of the product).  Its inverse by the
// lane-pair routine (fq6.go:295-336; one safegcd inversion, which does not split) on every pair alike, then conj(a) times it: one Fq6 product on
// each half.
BLSMI_NOINLINE Fp6S r_fp6_inv(const Fp6S n) { return fp6_store(fp6_inv(n)); }
BLSMI_NOINLINE R12 r12_inv(const R12 a) {
    R12 ac = a; r12_conj_inplace(ac);
    const R12 nn = r12_mul(a, ac);
    Fp6S n; n.c0 = fp2_store(bcast<0>(nn.c)); n.c1 = fp2_store(bcast<2>(nn.c)); n.c2 = fp2_store(bcast<4>(nn.c));
    const Fp6S t = r_fp6_inv(n);
    const auto tb = rsel<RQ0>(t.c0, rsel<RQ1>(t.c1, t.c2));                            // t_j in quad j, both pairs
    const auto p = fp2_norm(fp2_mul(ac.c, tb));
    const auto s = fp2_norm(fp2_mul(k6_sumop(ac.c), k6_sumop(tb)));
    R12 r;
    r.c = fp2_tight(k6_recombine(p, s));
    return r;
}
// fq12.go:171-177: conj^P on every coefficient, then w^p's factor gamma^p, gamma = xi^((q^P - 1) / 6): (xi^((q^P-1)/3))^j on the v-power (the
// tables of fq6.go:211-218) times gamma on the odd powers of w
template <int P>
BLSMI_DEV R12 r12_frob(const R12& a) {
    const Fp2S k6 = fp2_store(rsel<RQ0>(fp2_one(), rsel<RQ1>(BLSMI_FP2_K(C_FROB6_C1[P % 6]), BLSMI_FP2_K(C_FROB6_C2[P % 6]))));
    const Fp2S k12 = fp2_store(rsel<REVEN>(fp2_one(), BLSMI_FP2_K(C_FROB12_C1[P % 12])));
    R12 r;
    r.c = fp2_tight(fp2_mul(fp2_norm(fp2_mul(fp2_frob<P>(a.c), k6)), k12));
    return r;
}
BLSMI_NOINLINE R12 r12_frob1(const R12 a) { return r12_frob<1>(a); }
BLSMI_NOINLINE R12 r12_frob2(const R12 a) { return r12_frob<2>(a); }
BLSMI_NOINLINE R12 r12_frob3(const R12 a) { return r12_frob<3>(a); }
// the chain and the ExpByX loop of pairing_body.inc over R12: plain Granger-Scott squarings throughout (MIN_RUN = 0; see the head of this file)
BLSMI_NOINLINE R12 exp_by_x_r(const R12 f, u64 e);
struct RowOps {
    using T = R12;
    static constexpr int MIN_RUN = 0;
    static BLSMI_DEV void inv(T& r, const T& a) { r = r12_inv(a); }
    static BLSMI_DEV void mul(T& r, const T& a, const T& b) { r = r12_mul(a, b); }
    static BLSMI_DEV void cyc_sqr(T& r, const T& a) { r = r12_cyc_sqr(a); }
    static BLSMI_DEV void x_sqr(T& r, const T& a) { r = r12_cyc_sqr(a); }
    static BLSMI_DEV void frob1(T& r, const T& a) { r = r12_frob1(a); }
    static BLSMI_DEV void frob2(T& r, const T& a) { r = r12_frob2(a); }
    static BLSMI_DEV void frob3(T& r, const T& a) { r = r12_frob3(a); }
    static BLSMI_DEV void conj(T& a) { r12_conj_inplace(a); }
    static BLSMI_DEV void exp_x(T& r, const T& a, u64 e) { r = exp_by_x_r(a, e); }
};
BLSMI_NOINLINE R12 exp_by_x_r(const R12 f, u64 e) { R12 r; exp_by_x_loop<RowOps>(r, f, e); return r; }
BLSMI_DEV void final_exponentiation_r(R12& r) { final_exp_chain<RowOps>(r); }
