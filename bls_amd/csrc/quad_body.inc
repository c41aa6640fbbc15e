// quad_body.inc -- the pairing in the LANE-QUAD layout: FOUR adjacent lanes per tuple.  Lanes 4k, 4k+1 ("pair A") hold the Fq6 half c0
// of every Fq12 value, lanes 4k+2, 4k+3 ("pair B") the half c1; inside a pair the even lane holds c0 and the odd lane c1 of every Fq2
// (fp2_pair.inc, unchanged).  Included inside namespace blsmi::pairl after tower_body.inc / pairing_body.inc.
//
// Why: in the lane-pair layout 65 536 tuples fill the chip (1 024 SIMDs x 2 waves x 32 tuples); 16 384 tuples are 512 waves, half the
// SIMDs idle (pairings: 11.5 ms per 16 384 against 20.4 ms per 65 536, VERDICT r03 item 3).  Here 16 384 tuples are 1 024 waves, and a
// lane carries HALF the work: both pairs of a quad run the same instruction stream -- an Fq2 product, an Fq6 product -- on different
// operands, so an Fq12 squaring (two Fq6 products, fq12.go:180-195) costs ONE Fq6-product time, a sparse line multiplication
// (fq12.go:32-47) 8 Fq2-product times instead of 13, a Granger-Scott squaring 3 instead of 6, a compressed one 2 instead of 4.
// Values cross between the pairs through DPP quad_perm [2,3,0,1] (one v_mov_dpp per limb, no LDS); which operand a pair feeds into
// the shared stream is a per-lane v_bfi select.  Same field elements as the lane-pair routines: the Miller value differs from
// theirs in nothing (same homogeneous steps), the final exponentiation is the same chain.

#ifdef BLSMI_QUAD_INLINE
#define BLSMI_QFN BLSMI_DEV
#else
#define BLSMI_QFN BLSMI_NOINLINE
#endif
BLSMI_DEV i32 quad_hi() { return -(i32)((threadIdx.x >> 1) & 1); }                     // all-ones on pair B (lanes 2, 3 of the quad)
BLSMI_DEV i32 dpp_xpair(i32 x) { return __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xf, 0xf, true); }   // quad_perm [2,3,0,1]: the other pair's lane of the same parity
template <int L, int V> BLSMI_DEV Fp2<L, V> fp2_xchg(const Fp2<L, V>& a) {
    Fp2<L, V> r;
#pragma unroll
    for (int i = 0; i < NL; i++) r.c.v[i] = dpp_xpair(a.c.v[i]);
    return r;
}
template <int L, int V> BLSMI_DEV Fp6<L, V> fp6_xchg(const Fp6<L, V>& a) { Fp6<L, V> r; r.c0 = fp2_xchg(a.c0); r.c1 = fp2_xchg(a.c1); r.c2 = fp2_xchg(a.c2); return r; }
// per-pair choice: pair A's lanes get a, pair B's lanes get b (hi = quad_hi())
template <int La, int Va, int Lb, int Vb>
BLSMI_DEV auto fp2_ab(i32 hi, const Fp2<La, Va>& a, const Fp2<Lb, Vb>& b) {
    constexpr int L = imax(La, Lb), V = imax(Va, Vb);
    return fp2_select(hi, fp2_relabel<L, V>(b), fp2_relabel<L, V>(a));
}
template <int La, int Va, int Lb, int Vb>
BLSMI_DEV auto fp6_ab(i32 hi, const Fp6<La, Va>& a, const Fp6<Lb, Vb>& b) { return make_fp6(fp2_ab(hi, a.c0, b.c0), fp2_ab(hi, a.c1, b.c1), fp2_ab(hi, a.c2, b.c2)); }
template <int L, int V> BLSMI_DEV auto fp2_cneg(i32 m, const Fp2<L, V>& a) { return wrap(fp_cneg(m, a.c)); }      // m ? -a : a

// An Fq12 value of one tuple: pair A's h is c0, pair B's h is c1 (45 words per lane; the lane-pair layout needs 90)
struct Q12 { Fp6S h; };
BLSMI_DEV Q12 q12_one() { Q12 r; r.h.c0 = fp2_select(quad_hi(), fp2_zero(), fp2_one()); r.h.c1 = fp2_zero(); r.h.c2 = fp2_zero(); return r; }
BLSMI_DEV void q12_conj_inplace(Q12& a) {                                              // fq12.go:27-29: c1 = -c1 (pair B)
    const i32 hi = quad_hi();
    a.h.c0 = fp2_cneg(hi, a.h.c0); a.h.c1 = fp2_cneg(hi, a.h.c1); a.h.c2 = fp2_cneg(hi, a.h.c2);
}
// from / to the lane-pair form of the same value (both pairs of the quad hold all of it)
BLSMI_DEV Q12 q12_from_pair(const Fp12S& f) { Q12 r; r.h = fp6_store(fp6_ab(quad_hi(), f.c0, f.c1)); return r; }
BLSMI_DEV Fp12S q12_to_pair(const Q12& a) {
    const Fp6S o = fp6_xchg(a.h);
    const i32 hi = quad_hi();
    Fp12S r; r.c0 = fp6_store(fp6_ab(hi, a.h, o)); r.c1 = fp6_store(fp6_ab(hi, o, a.h));
    return r;
}

// fq12.go:180-195.  ab = a0 a1, t = (a0 + v a1)(a0 + a1); c0 = t - ab - v ab, c1 = 2 ab: pair A multiplies t, pair B multiplies ab
BLSMI_QFN void q12_sqr(Q12& r, const Q12& a) {
    const i32 hi = quad_hi();
    const Fp6S o = fp6_xchg(a.h);                                                      // A: a1    B: a0
    const auto X = fp6_ab(hi, fp6_add(a.h, fp6_mul_nr(o)), o);
    const auto Y = fp6_ab(hi, fp6_add(a.h, o), a.h);
    const auto P = fp6_norm(fp6_mul(X, Y));                                            // A: t     B: ab
    const auto Po = fp6_xchg(P);                                                       // A: ab
    r.h = fp6_store(fp6_ab(hi, fp6_sub(fp6_sub(P, Po), fp6_mul_nr(Po)), fp6_add(P, P)));
}
// fq12.go:198-213, Karatsuba over the two pairs: c0 = a0 b0 + v a1 b1, c1 = (a0 + a1)(b0 + b1) - a0 b0 - a1 b1.  Pair A multiplies a0 b0,
// pair B a1 b1 (one Fq6-product time); the third Fq6 product's six Fq2 products (fq6.go:255-292) are split three and three -- A the plain
// ones X_i Y_i, B the sums' (X_i + X_j)(Y_i + Y_j) -- and meet on pair B, where c1 lives: 9 product times against 18 in a lane pair
// (the four half products a0 b0, a1 b1, a0 b1, a1 b0 would be 12).
BLSMI_QFN void q12_mul(Q12& r, const Q12& a, const Q12& b) {
    const i32 hi = quad_hi();
    const Fp6S ao = fp6_xchg(a.h), bo = fp6_xchg(b.h);
    const auto R1 = fp6_norm(fp6_mul(a.h, b.h));                                       // A: a0 b0   B: a1 b1
    const Fp6S X = fp6_store(fp6_add(a.h, ao)), Y = fp6_store(fp6_add(b.h, bo));      // a0 + a1, b0 + b1 on both pairs
    const auto p0 = fp2_norm(fp2_mul(fp2_ab(hi, X.c0, fp2_add(X.c1, X.c2)), fp2_ab(hi, Y.c0, fp2_add(Y.c1, Y.c2))));   // A: X0 Y0   B: (X1+X2)(Y1+Y2)
    const auto p1 = fp2_norm(fp2_mul(fp2_ab(hi, X.c1, fp2_add(X.c0, X.c2)), fp2_ab(hi, Y.c1, fp2_add(Y.c0, Y.c2))));   // A: X1 Y1   B: (X0+X2)(Y0+Y2)
    const auto p2 = fp2_norm(fp2_mul(fp2_ab(hi, X.c2, fp2_add(X.c0, X.c1)), fp2_ab(hi, Y.c2, fp2_add(Y.c0, Y.c1))));   // A: X2 Y2   B: (X0+X1)(Y0+Y1)
    const auto aa = fp2_xchg(p0), bb = fp2_xchg(p1), cc = fp2_xchg(p2);                // on pair B: A's plain products
    // pair B: T = (a0 + a1)(b0 + b1) as fq6.go:255-292 puts it together (pair A evaluates the same expressions on swapped data and drops them)
    const auto t1 = fp2_add(fp2_mul_nr(fp2_sub(fp2_sub(p0, bb), cc)), aa);
    const auto t3 = fp2_sub(fp2_add(fp2_sub(p1, aa), bb), cc);
    const auto t2 = fp2_add(fp2_sub(fp2_sub(p2, aa), bb), fp2_mul_nr(cc));
    const auto T = make_fp6(t1, t2, t3);
    const auto R1o = fp6_xchg(R1);                                                     // A: a1 b1   B: a0 b0
    r.h = fp6_store(fp6_ab(hi, fp6_add(R1, fp6_mul_nr(R1o)), fp6_sub(fp6_sub(T, R1), R1o)));
}
// fq12.go:32-47: a * (c0 + c1 v + c4 v w) = [a0 L0 + v (a1 L1)] + [a0 L1 + a1 L0] w with L0 = c0 + c1 v, L1 = c4 v:
// both pairs run MulBy01 on their own half and MulBy1 on the other pair's -- 5 + 3 products against 13
template <int L0, int V0, int L1, int V1, int L4, int V4>
BLSMI_DEV Q12 q12_mul_by_014(const Q12& a, const Fp2<L0, V0>& c0, const Fp2<L1, V1>& c1, const Fp2<L4, V4>& c4) {
    const i32 hi = quad_hi();
    const Fp6S o = fp6_xchg(a.h);
    const auto R1 = fp6_norm(fp6_mul_by_01(a.h, c0, c1));                              // A: a0 L0   B: a1 L0
    const auto R2 = fp6_norm(fp6_mul_by_1(o, c4));                                     // A: a1 L1   B: a0 L1
    Q12 r;
    r.h = fp6_store(fp6_ab(hi, fp6_add(R1, fp6_mul_nr(R2)), fp6_add(R1, R2)));
    return r;
}
// fq12.go:216-237: t = (a0^2 - v a1^2)^-1 (both pairs), c0 = t a0, c1 = -t a1
BLSMI_NOINLINE void q12_inv(Q12& r, const Q12& a) {
    const i32 hi = quad_hi();
    const Fp6S S = fp6_store(fp6_sqr(a.h));                                            // A: a0^2   B: a1^2
    const Fp6S So = fp6_xchg(S);
    const Fp6S t = fp6_store(fp6_inv(fp6_store(fp6_ab(hi, fp6_sub(S, fp6_mul_nr(So)), fp6_sub(So, fp6_mul_nr(S))))));
    const auto P = fp6_norm(fp6_mul(t, a.h));
    r.h = fp6_store(fp6_ab(hi, P, fp6_neg(P)));
}
// fq12.go:171-177: Frobenius on both halves, then c1 times (1+u)^((q^P-1)/6) (pair B; pair A multiplies by one)
template <int P>
BLSMI_DEV void q12_frob(Q12& r, const Q12& a) {
    const Fp6S c = fp6_store(fp6_frob<P>(a.h));
    const Fp2S k = fp2_select(quad_hi(), BLSMI_FP2_K(C_FROB12_C1[P % 12]), fp2_one());
    r.h = fp6_store(make_fp6(fp2_mul(c.c0, k), fp2_mul(c.c1, k), fp2_mul(c.c2, k)));
}
BLSMI_NOINLINE void q12_frob1(Q12& r, const Q12& a) { q12_frob<1>(r, a); }
BLSMI_NOINLINE void q12_frob2(Q12& r, const Q12& a) { q12_frob<2>(r, a); }
BLSMI_NOINLINE void q12_frob3(Q12& r, const Q12& a) { q12_frob<3>(r, a); }
BLSMI_DEV bool q12_is_one(const Q12& a) {
    const Fp2S w = fp2_select(quad_hi(), fp2_zero(), fp2_one());
    int e = (fp2_eq(a.h.c0, w) & fp2_is_zero(a.h.c1) & fp2_is_zero(a.h.c2)) ? 1 : 0;
    return (e & __shfl_xor(e, 2)) != 0;
}

// ---- one Fq4 squaring shared by the two pairs: (p + q w)^2 with w^2 = xi is (t - v - xi v) + 2 v w with v = p q,
// t = (p + q)(p + xi q).  Pair A multiplies t, pair B multiplies v, and v crosses to A: `first` is valid on pair A's lanes,
// `second` on pair B's.
struct Q4 { Fp2S first, second; };
template <int La, int Va, int Lb, int Vb>
BLSMI_DEV Q4 q4_sqr(i32 hi, const Fp2<La, Va>& p, const Fp2<Lb, Vb>& q) {
    const auto X = fp2_ab(hi, fp2_add(p, q), p);
    const auto Y = fp2_ab(hi, fp2_add(p, fp2_mul_nr(q)), q);
    const auto P = fp2_norm(fp2_mul(X, Y));                                            // A: t   B: v
    const auto vo = fp2_xchg(P);                                                       // A: v
    Q4 r;
    r.first = fp2_store(fp2_sub(fp2_sub(P, vo), fp2_mul_nr(vo)));
    r.second = fp2_store(fp2_dbl(P));
    return r;
}
// Granger-Scott squaring on the cyclotomic subgroup (tower_body.inc: fp12_cyclotomic_sqr) -- z0 z4 z3 live on pair A, z2 z1 z5 on B;
// every Fq4 (z0,z1), (z2,z3), (z4,z5) has one coefficient on each side.  Three product times against six.
BLSMI_QFN void q12_cyc_sqr(Q12& r, const Q12& f) {
    const i32 hi = quad_hi();
    const Fp6S& h = f.h;
    const Fp6S o = fp6_xchg(h);
    const Q4 a = q4_sqr(hi, fp2_ab(hi, h.c0, o.c0), fp2_ab(hi, o.c1, h.c1));           // (z0, z1)
    const Q4 b = q4_sqr(hi, fp2_ab(hi, o.c0, h.c0), fp2_ab(hi, h.c2, o.c2));           // (z2, z3)
    const Q4 c = q4_sqr(hi, fp2_ab(hi, h.c1, o.c1), fp2_ab(hi, o.c2, h.c2));           // (z4, z5)
    // A: (3 a.first - 2 z0, 3 b.first - 2 z4, 3 c.first - 2 z3)      B: (3 xi c.second + 2 z2, 3 a.second + 2 z1, 3 b.second + 2 z5)
    const auto w0 = fp2_ab(hi, a.first, fp2_mul_nr(c.second));
    const auto w1 = fp2_ab(hi, b.first, a.second);
    const auto w2 = fp2_ab(hi, c.first, b.second);
    const i32 lo = ~hi;                                                                // negate the old coefficient on pair A
    r.h.c0 = fp2_store(fp2_add(fp2_dbl(fp2_add(w0, fp2_cneg(lo, h.c0))), w0));
    r.h.c1 = fp2_store(fp2_add(fp2_dbl(fp2_add(w1, fp2_cneg(lo, h.c1))), w1));
    r.h.c2 = fp2_store(fp2_add(fp2_dbl(fp2_add(w2, fp2_cneg(lo, h.c2))), w2));
}
// Karabina's compressed form of a run of squarings (tower_body.inc: cyc_compressed_sqr): pair A carries u = z4, w = z3, pair B
// u = z2, w = z5.  Two product times per squaring against four.
struct QC { Fp2S u, w; };
BLSMI_DEV QC qc_compress(const Q12& f) { QC c; c.u = fp2_select(quad_hi(), f.h.c0, f.h.c1); c.w = f.h.c2; return c; }
BLSMI_DEV QC qc_sqr(const QC& g) {
    const i32 hi = quad_hi();
    const Fp2S ou = fp2_xchg(g.u), ow = fp2_xchg(g.w);
    const Q4 b = q4_sqr(hi, fp2_ab(hi, ou, g.u), fp2_ab(hi, g.w, ow));                 // (z2, z3)
    const Q4 c = q4_sqr(hi, fp2_ab(hi, g.u, ou), fp2_ab(hi, ow, g.w));                 // (z4, z5)
    // A: z4' = 3 b.first - 2 z4, z3' = 3 c.first - 2 z3       B: z2' = 3 xi c.second + 2 z2, z5' = 3 b.second + 2 z5
    const auto wu = fp2_ab(hi, b.first, fp2_mul_nr(c.second));
    const auto ww = fp2_ab(hi, c.first, b.second);
    const i32 lo = ~hi;
    QC r;
    r.u = fp2_store(fp2_add(fp2_dbl(fp2_add(wu, fp2_cneg(lo, g.u))), wu));
    r.w = fp2_store(fp2_add(fp2_dbl(fp2_add(ww, fp2_cneg(lo, g.w))), ww));
    return r;
}
// the end of a compressed run: both pairs rebuild (z2, z3, z4, z5), recover z1 and z0 with the lane-pair routines (one safegcd
// inversion, which does not split) and keep their half
BLSMI_NOINLINE void q12_cyc_sqr_run(Q12& r, const Q12& g, int m) {
    QC c = qc_compress(g);
    for (int j = 0; j < m; j++) c = qc_sqr(c);
    const i32 hi = quad_hi();
    const Fp2S ou = fp2_xchg(c.u), ow = fp2_xchg(c.w);
    CycCompressed full;
    full.z4 = fp2_store(fp2_ab(hi, c.u, ou)); full.z3 = fp2_store(fp2_ab(hi, c.w, ow));
    full.z2 = fp2_store(fp2_ab(hi, ou, c.u)); full.z5 = fp2_store(fp2_ab(hi, ow, c.w));
    Fp2S num, den;
    cyc_z1_fraction(full, num, den);
    const Fp12S d = cyc_decompress(full, fp2_store(fp2_mul(num, fp2_store(fp2_inv(den)))));
    r.h = fp6_store(fp6_ab(hi, d.c0, d.c1));
}

// ---- Miller loop (pairing.go:16-75) with the homogeneous steps of pairing_body.inc.  The running point is held by BOTH pairs;
// the nine Fq2 products of a doubling step run as five product times: two products and three squarings, each pair its own.
BLSMI_QFN void doubling_step_q(G2Proj& r, Fp2S& o0, Fp2S& o1, Fp2S& o2) {
    const i32 hi = quad_hi();
    const auto M1 = fp2_norm(fp2_mul(fp2_ab(hi, r.x, r.y), fp2_ab(hi, r.y, r.z)));     // A: XY      B: YZ
    const auto S1 = fp2_norm(fp2_sqr(fp2_ab(hi, r.y, r.x)));                           // A: Y^2     B: X^2
    const auto Z2 = fp2_norm(fp2_sqr(r.z));
    const auto M1o = fp2_xchg(M1), S1o = fp2_xchg(S1);
    const auto A = fp2_ab(hi, M1, M1o), YZ = fp2_ab(hi, M1o, M1);
    const auto B = fp2_ab(hi, S1, S1o), X2 = fp2_ab(hi, S1o, S1);
    const auto H = fp2_norm(fp2_dbl(YZ));
    const auto E = fp2_norm(fp2_muls<12>(fp2_norm(fp2_mul_nr(Z2))));
    const auto F = fp2_norm(fp2_muls<3>(E));
    const auto G = fp2_norm(fp2_add(B, F));
    const auto M2 = fp2_norm(fp2_mul(fp2_ab(hi, A, B), fp2_ab(hi, fp2_norm(fp2_sub(B, F)), H)));   // A: A (B - F)    B: B H
    const auto S2 = fp2_norm(fp2_sqr(fp2_ab(hi, G, E)));                               // A: G^2     B: E^2
    const auto M2o = fp2_xchg(M2), S2o = fp2_xchg(S2);
    const auto nx = fp2_dbl(fp2_ab(hi, M2, M2o));
    const auto nz = fp2_muls<4>(fp2_ab(hi, M2o, M2));
    const auto ny = fp2_sub(fp2_ab(hi, S2, S2o), fp2_muls<12>(fp2_ab(hi, S2o, S2)));
    o2 = fp2_store(fp2_sub(B, E));
    o1 = fp2_store(fp2_neg(fp2_muls<3>(X2)));
    o0 = fp2_store(H);
    r.x = fp2_store(nx); r.y = fp2_store(ny); r.z = fp2_store(nz);
}
// the line (o0, o1, o2) evaluated at P: o2 + (o1 P.x) v + (o0 P.y) v w (pairing.go:28-39); pair A scales o0, pair B o1
BLSMI_DEV void line_at_q(const Fp2S& o0, const Fp2S& o1, const FpS& px, const FpS& py, Fp2S& c0, Fp2S& c1) {
    const i32 hi = quad_hi();
    const Fp2S s = fp2_store(fp2_mul_fp(fp2_select(hi, o1, o0), fp_select(hi, px, py)));   // A: o0 P.y   B: o1 P.x
    const Fp2S so = fp2_xchg(s);
    c0 = fp2_select(hi, so, s); c1 = fp2_select(hi, s, so);
}
BLSMI_QFN void ell_q(Q12& f, const Fp2S& o0, const Fp2S& o1, const Fp2S& o2, const FpS& px, const FpS& py) {
    Fp2S c0, c1;
    line_at_q(o0, o1, px, py, c0, c1);
    f = q12_mul_by_014(f, o2, c1, c0);
}
BLSMI_QFN void ell_sqr_q(Q12& f, const Fp2S& o0, const Fp2S& o1, const Fp2S& o2, const FpS& px, const FpS& py) {
    Fp2S c0, c1;
    line_at_q(o0, o1, px, py, c0, c1);
    const Q12 g = q12_mul_by_014(f, o2, c1, c0);
    q12_sqr(f, g);
}
// one (P, Q) pair, homogeneous steps: the value k_miller1h_pair computes (a Miller value up to factors the final exponentiation
// removes).  The five addition steps are run by both pairs alike.
BLSMI_DEV void miller_loop_q(Q12& f, const FpS& px, const FpS& py, const Fp2S& qx, const Fp2S& qy) {
    G2Proj r; r.x = qx; r.y = qy; r.z = fp2_one();
    f = q12_one();
    Fp2S o0, o1, o2;
    x_bit_walk([&] { doubling_step_q(r, o0, o1, o2); },
               [&] { addition_step_h(r, qx, qy, o0, o1, o2); },
               [&] { ell_q(f, o0, o1, o2, px, py); },
               [&] { ell_sqr_q(f, o0, o1, o2, px, py); });
    q12_conj_inplace(f);                                                               // blsIsNegative (pairing.go:71-73)
}

// ---- two (P, Q) pairs sharing the squarings (CompareTwoPairings, pairing.go:140-147; the verify family).  As in the lane-pair loop
// the two lines of a step are multiplied together first (tower_body.inc: line_pair_product, six independent products: three per
// pair here) and the 5-coefficient result goes into f as [f0 M0 + v f1 M1] + [f0 M1 + f1 M0] w with M0 = l0 + l1 v + l2 v^2,
// M1 = l4 v + l5 v^2 -- by Karatsuba over the two pairs (ell2_q): 9 product times against 17.
BLSMI_DEV LinePair line_pair_product_q(const Fp2S& a0, const Fp2S& a1, const Fp2S& a4, const Fp2S& b0, const Fp2S& b1, const Fp2S& b4) {
    const i32 hi = quad_hi();
    // A: a0 b0, a1 b1, a4 b4        B: (a0+a1)(b0+b1), (a0+a4)(b0+b4), (a1+a4)(b1+b4)
    const auto r1 = fp2_norm(fp2_mul(fp2_ab(hi, a0, fp2_add(a0, a1)), fp2_ab(hi, b0, fp2_add(b0, b1))));
    const auto r2 = fp2_norm(fp2_mul(fp2_ab(hi, a1, fp2_add(a0, a4)), fp2_ab(hi, b1, fp2_add(b0, b4))));
    const auto r3 = fp2_norm(fp2_mul(fp2_ab(hi, a4, fp2_add(a1, a4)), fp2_ab(hi, b4, fp2_add(b1, b4))));
    const auto r1o = fp2_xchg(r1), r2o = fp2_xchg(r2), r3o = fp2_xchg(r3);
    const auto p00 = fp2_ab(hi, r1, r1o), s01 = fp2_ab(hi, r1o, r1);
    const auto p11 = fp2_ab(hi, r2, r2o), s04 = fp2_ab(hi, r2o, r2);
    const auto p44 = fp2_ab(hi, r3, r3o), s14 = fp2_ab(hi, r3o, r3);
    LinePair r;
    r.l0 = fp2_store(fp2_add(p00, fp2_mul_nr(p44)));
    r.l1 = fp2_store(fp2_sub(fp2_sub(s01, p00), p11));
    r.l2 = fp2_store(p11);
    r.l4 = fp2_store(fp2_sub(fp2_sub(s04, p00), p44));
    r.l5 = fp2_store(fp2_sub(fp2_sub(s14, p11), p44));
    return r;
}
template <bool SQR>
BLSMI_QFN void ell2_q(Q12& f, const Fp2S& a0, const Fp2S& a1, const Fp2S& a2, const FpS& ax, const FpS& ay,
                      const Fp2S& b0, const Fp2S& b1, const Fp2S& b2, const FpS& bx, const FpS& by) {
    const i32 hi = quad_hi();
    // the four scalings by P.x / P.y: pair A takes line a's, pair B line b's
    const Fp2S s1 = fp2_store(fp2_mul_fp(fp2_select(hi, b1, a1), fp_select(hi, bx, ax)));
    const Fp2S s0 = fp2_store(fp2_mul_fp(fp2_select(hi, b0, a0), fp_select(hi, by, ay)));
    const Fp2S s1o = fp2_xchg(s1), s0o = fp2_xchg(s0);
    const LinePair m = line_pair_product_q(a2, fp2_select(hi, s1o, s1), fp2_select(hi, s0o, s0), b2, fp2_select(hi, s1, s1o), fp2_select(hi, s0, s0o));
    // f (M0 + M1 w) with M0 = l0 + l1 v + l2 v^2, M1 = l4 v + l5 v^2, Karatsuba over the two pairs as in q12_mul: A multiplies f0 M0, B f1 M1
    // (one Fq6-product time), the six Fq2 products of (f0 + f1)(M0 + M1) go three and three and meet on pair B: 9 product times (lane pair: 17)
    const Fp6S o = fp6_xchg(f.h);
    const Fp6S mm = fp6_store(fp6_ab(hi, make_fp6(m.l0, m.l1, m.l2), make_fp6(fp2_zero(), m.l4, m.l5)));
    const auto R1 = fp6_norm(fp6_mul(f.h, mm));                                        // A: f0 M0   B: f1 M1
    const Fp6S X = fp6_store(fp6_add(f.h, o));
    const Fp6S Y = fp6_store(make_fp6(m.l0, fp2_add(m.l1, m.l4), fp2_add(m.l2, m.l5)));
    const auto p0 = fp2_norm(fp2_mul(fp2_ab(hi, X.c0, fp2_add(X.c1, X.c2)), fp2_ab(hi, Y.c0, fp2_add(Y.c1, Y.c2))));
    const auto p1 = fp2_norm(fp2_mul(fp2_ab(hi, X.c1, fp2_add(X.c0, X.c2)), fp2_ab(hi, Y.c1, fp2_add(Y.c0, Y.c2))));
    const auto p2 = fp2_norm(fp2_mul(fp2_ab(hi, X.c2, fp2_add(X.c0, X.c1)), fp2_ab(hi, Y.c2, fp2_add(Y.c0, Y.c1))));
    const auto aa = fp2_xchg(p0), bb = fp2_xchg(p1), cc = fp2_xchg(p2);
    const auto t1 = fp2_add(fp2_mul_nr(fp2_sub(fp2_sub(p0, bb), cc)), aa);
    const auto t3 = fp2_sub(fp2_add(fp2_sub(p1, aa), bb), cc);
    const auto t2 = fp2_add(fp2_sub(fp2_sub(p2, aa), bb), fp2_mul_nr(cc));
    const auto T = make_fp6(t1, t2, t3);
    const auto R1o = fp6_xchg(R1);
    Q12 g;
    g.h = fp6_store(fp6_ab(hi, fp6_add(R1, fp6_mul_nr(R1o)), fp6_sub(fp6_sub(T, R1), R1o)));
    if (SQR) q12_sqr(f, g); else f = g;
}
// PRE0: pair 0's G2 point is the generator, its 68 line triples are read from `pre` (pairing_body.inc: load_line); pair 1 by the
// homogeneous steps.  Without PRE0 both points run their steps -- the doubling steps one after the other in the shared-stream form,
// the five addition steps SIDE BY SIDE: pair A adds on point 0 while pair B adds on point 1 (one instruction stream, the lane-pair
// routine), and the lines cross.
template <bool PRE0>
BLSMI_DEV void miller_loop2_q(Q12& f, const FpS (&px)[2], const FpS (&py)[2], const Fp2S (&qx)[2], const Fp2S (&qy)[2], const i32* pre) {
    const i32 hi = quad_hi();
    G2Proj r0, r1;
    r0.x = qx[0]; r0.y = qy[0]; r0.z = fp2_one();
    r1.x = qx[1]; r1.y = qy[1]; r1.z = fp2_one();
    f = q12_one();
    Fp2S o0, o1, o2, n0, n1, n2;
    int line = 0;
    auto add_both = [&]() {
        if (PRE0) { load_line(pre, line++, o0, o1, o2); addition_step_h(r1, qx[1], qy[1], n0, n1, n2); return; }
        // A works on point 0, B on point 1; afterwards each pair holds its own point's successor and line, the other's through DPP
        G2Proj t; t.x = fp2_select(hi, r1.x, r0.x); t.y = fp2_select(hi, r1.y, r0.y); t.z = fp2_select(hi, r1.z, r0.z);
        Fp2S m0, m1, m2;
        addition_step_h(t, fp2_select(hi, qx[1], qx[0]), fp2_select(hi, qy[1], qy[0]), m0, m1, m2);
        const Fp2S tx = fp2_xchg(t.x), ty = fp2_xchg(t.y), tz = fp2_xchg(t.z), k0 = fp2_xchg(m0), k1 = fp2_xchg(m1), k2 = fp2_xchg(m2);
        r0.x = fp2_select(hi, tx, t.x); r0.y = fp2_select(hi, ty, t.y); r0.z = fp2_select(hi, tz, t.z);
        r1.x = fp2_select(hi, t.x, tx); r1.y = fp2_select(hi, t.y, ty); r1.z = fp2_select(hi, t.z, tz);
        o0 = fp2_select(hi, k0, m0); o1 = fp2_select(hi, k1, m1); o2 = fp2_select(hi, k2, m2);
        n0 = fp2_select(hi, m0, k0); n1 = fp2_select(hi, m1, k1); n2 = fp2_select(hi, m2, k2);
    };
    x_bit_walk([&] { if (PRE0) load_line(pre, line++, o0, o1, o2); else doubling_step_q(r0, o0, o1, o2);
                     doubling_step_q(r1, n0, n1, n2); },
               add_both,
               [&] { ell2_q<false>(f, o0, o1, o2, px[0], py[0], n0, n1, n2, px[1], py[1]); },
               [&] { ell2_q<true>(f, o0, o1, o2, px[0], py[0], n0, n1, n2, px[1], py[1]); });
    q12_conj_inplace(f);
}

// ---- final exponentiation (pairing.go:79-129): the chain and the ExpByX loop of pairing_body.inc over Q12.  The routines above write their
// result while they still read their operands, so each goes through a temporary.
BLSMI_NOINLINE void exp_by_x_q(Q12& out, const Q12& f, u64 e);
struct QuadOps {
    using T = Q12;
    // measured at 16 384 pairings (tools/ab_bench.py): the 16-squaring run of |x| NOT compressed 4.05 -> 3.95 ms for the final exponentiation
    // (a decompression -- one inversion, which does not split over the pairs -- outweighs 16 x (3 - 2) products here); the run of 32 stays compressed
    static constexpr int MIN_RUN = 27;
    static BLSMI_DEV void inv(T& r, const T& a) { T t; q12_inv(t, a); r = t; }
    static BLSMI_DEV void mul(T& r, const T& a, const T& b) { T t; q12_mul(t, a, b); r = t; }
    static BLSMI_DEV void cyc_sqr(T& r, const T& a) { T t; q12_cyc_sqr(t, a); r = t; }
    static BLSMI_DEV void x_sqr(T& r, const T& a) { cyc_sqr(r, a); }
    static BLSMI_DEV void x_sqr_run(T& r, const T& a, int m) { T t; q12_cyc_sqr_run(t, a, m); r = t; }
    static BLSMI_DEV void frob1(T& r, const T& a) { T t; q12_frob1(t, a); r = t; }
    static BLSMI_DEV void frob2(T& r, const T& a) { T t; q12_frob2(t, a); r = t; }
    static BLSMI_DEV void frob3(T& r, const T& a) { T t; q12_frob3(t, a); r = t; }
    static BLSMI_DEV void conj(T& a) { q12_conj_inplace(a); }
    static BLSMI_DEV void exp_x(T& r, const T& a, u64 e) { exp_by_x_q(r, a, e); }
};
BLSMI_NOINLINE void exp_by_x_q(Q12& out, const Q12& f, u64 e) { exp_by_x_loop<QuadOps>(out, f, e); }
BLSMI_DEV void final_exponentiation_q(Q12& r) { final_exp_chain<QuadOps>(r); }
