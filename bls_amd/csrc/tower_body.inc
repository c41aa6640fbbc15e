// tower_body.inc -- Fq6 / Fq12 over an Fq2 layer given by the including namespace (fp2_single.inc or
// fp2_pair.inc): fq6.go:34-336, fq12.go:27-237 restated once for both lane layouts.
template <int L2, int V2, int L, int V>
BLSMI_DEV Fp6<L2, V2> fp6_relabel(const Fp6<L, V>& a) {
    Fp6<L2, V2> r;
    r.c0 = fp2_relabel<L2, V2>(a.c0);
    r.c1 = fp2_relabel<L2, V2>(a.c1);
    r.c2 = fp2_relabel<L2, V2>(a.c2);
    return r;
}
template <int La, int Va, int Lb, int Vb, int Lc, int Vc>
BLSMI_DEV auto make_fp6(const Fp2<La, Va>& a, const Fp2<Lb, Vb>& b, const Fp2<Lc, Vc>& c) {
    constexpr int L = imax(La, imax(Lb, Lc)), V = imax(Va, imax(Vb, Vc));
    Fp6<L, V> r;
    r.c0 = fp2_relabel<L, V>(a);
    r.c1 = fp2_relabel<L, V>(b);
    r.c2 = fp2_relabel<L, V>(c);
    return r;
}
template <int La, int Va, int Lb, int Vb>
BLSMI_DEV auto make_fp12(const Fp6<La, Va>& a, const Fp6<Lb, Vb>& b) {
    constexpr int L = imax(La, Lb), V = imax(Va, Vb);
    Fp12<L, V> r;
    r.c0 = fp6_relabel<L, V>(a);
    r.c1 = fp6_relabel<L, V>(b);
    return r;
}

// ------------------------------------------------------------------------------------------------
// Fq6
// ------------------------------------------------------------------------------------------------
template <int La, int Va, int Lb, int Vb> BLSMI_DEV auto fp6_add(const Fp6<La, Va>& a, const Fp6<Lb, Vb>& b) { return make_fp6(fp2_add(a.c0, b.c0), fp2_add(a.c1, b.c1), fp2_add(a.c2, b.c2)); }
template <int La, int Va, int Lb, int Vb> BLSMI_DEV auto fp6_sub(const Fp6<La, Va>& a, const Fp6<Lb, Vb>& b) { return make_fp6(fp2_sub(a.c0, b.c0), fp2_sub(a.c1, b.c1), fp2_sub(a.c2, b.c2)); }
template <int L, int V> BLSMI_DEV auto fp6_neg(const Fp6<L, V>& a) { return make_fp6(fp2_neg(a.c0), fp2_neg(a.c1), fp2_neg(a.c2)); }
template <int L, int V> BLSMI_DEV auto fp6_norm(const Fp6<L, V>& a) { return make_fp6(fp2_norm(a.c0), fp2_norm(a.c1), fp2_norm(a.c2)); }
template <int L, int V> BLSMI_DEV Fp6S fp6_store(const Fp6<L, V>& a) { Fp6S r; r.c0 = fp2_store(a.c0); r.c1 = fp2_store(a.c1); r.c2 = fp2_store(a.c2); return r; }
template <int L, int V> BLSMI_DEV Fp6R fp6_reduced(const Fp6<L, V>& a) { Fp6R r; r.c0 = fp2_reduced(a.c0); r.c1 = fp2_reduced(a.c1); r.c2 = fp2_reduced(a.c2); return r; }
// fp2_as<F2>(x): x in the type F2 a routine's values travel in -- the reduced type (fp_reduced) or the storage type (fp_store)
template <class F2, int L, int V> BLSMI_DEV F2 fp2_as(const Fp2<L, V>& a) {
    static_assert(std::is_same<F2, Fp2R>::value || std::is_same<F2, Fp2S>::value, "the reduced or the storage type");
    if constexpr (std::is_same<F2, Fp2R>::value) return fp2_reduced(a); else return fp2_store(a);
}
template <int L, int V> BLSMI_DEV Fp2W fp2_work(const Fp2<L, V>& a) { return fp2_as<Fp2W>(a); }
// fp2_trim(x): a small multiple that is about to be used several times -- with 28-bit limbs value-reduced once, here, instead of once per
// use; with 27-bit limbs, where no use would reduce it, only normalised
template <int L, int V> BLSMI_DEV auto fp2_trim(const Fp2<L, V>& a) {
#ifdef BLSMI_LIMBS28
    return fp2_reduced(a);
#else
    return fp2_norm(a);
#endif
}
template <int L, int V> BLSMI_DEV Fp6W fp6_work(const Fp6<L, V>& a) { Fp6W r; r.c0 = fp2_work(a.c0); r.c1 = fp2_work(a.c1); r.c2 = fp2_work(a.c2); return r; }
BLSMI_DEV Fp6S fp6_zero() { Fp6S r; r.c0 = fp2_zero(); r.c1 = fp2_zero(); r.c2 = fp2_zero(); return r; }
BLSMI_DEV Fp6S fp6_one() { Fp6S r; r.c0 = fp2_one(); r.c1 = fp2_zero(); r.c2 = fp2_zero(); return r; }
// fq6.go:34-37: multiply by v
template <int L, int V> BLSMI_DEV auto fp6_mul_nr(const Fp6<L, V>& a) { return make_fp6(fp2_mul_nr(a.c2), a.c0, a.c1); }
// fq6.go:255-292
template <int La, int Va, int Lb, int Vb>
BLSMI_DEV auto fp6_mul(const Fp6<La, Va>& a, const Fp6<Lb, Vb>& b) {
    const auto aa = fp2_mul(a.c0, b.c0);
    const auto bb = fp2_mul(a.c1, b.c1);
    const auto cc = fp2_mul(a.c2, b.c2);
    const auto t1 = fp2_add(fp2_mul_nr(fp2_sub(fp2_sub(fp2_mul(fp2_add(b.c1, b.c2), fp2_add(a.c1, a.c2)), bb), cc)), aa);
    const auto t3 = fp2_sub(fp2_add(fp2_sub(fp2_mul(fp2_add(b.c0, b.c2), fp2_add(a.c0, a.c2)), aa), bb), cc);
    const auto t2 = fp2_add(fp2_sub(fp2_sub(fp2_mul(fp2_add(b.c0, b.c1), fp2_add(a.c0, a.c1)), aa), bb), fp2_mul_nr(cc));
    return make_fp6(t1, t2, t3);
}
// fq6.go:221-252
template <int L, int V>
BLSMI_DEV auto fp6_sqr(const Fp6<L, V>& a) {
    const auto s0 = fp2_sqr(a.c0);
    const auto s1 = fp2_dbl(fp2_mul(a.c0, a.c1));
    const auto s2 = fp2_sqr(fp2_add(fp2_sub(a.c0, a.c1), a.c2));
    const auto s3 = fp2_dbl(fp2_mul(a.c1, a.c2));
    const auto s4 = fp2_sqr(a.c2);
    const auto c0 = fp2_add(fp2_mul_nr(s3), s0);
    const auto c1 = fp2_add(fp2_mul_nr(s4), s1);
    const auto c2 = fp2_sub(fp2_sub(fp2_add(fp2_add(s1, s2), s3), s0), s4);
    return make_fp6(c0, c1, c2);
}
// fq6.go:40-57
template <int L, int V, int Lc, int Vc>
BLSMI_DEV auto fp6_mul_by_1(const Fp6<L, V>& a, const Fp2<Lc, Vc>& c1) {
    const auto b = fp2_mul(a.c1, c1);
    const auto t1 = fp2_mul_nr(fp2_sub(fp2_mul(c1, fp2_add(a.c1, a.c2)), b));
    const auto t2 = fp2_sub(fp2_mul(c1, fp2_add(a.c0, a.c1)), b);
    return make_fp6(t1, t2, b);
}
// fq6.go:60-90
template <int L, int V, int L0, int V0, int L1, int V1>
BLSMI_DEV auto fp6_mul_by_01(const Fp6<L, V>& a, const Fp2<L0, V0>& c0, const Fp2<L1, V1>& c1) {
    const auto aa = fp2_mul(a.c0, c0);
    const auto b = fp2_mul(a.c1, c1);
    const auto t1 = fp2_add(fp2_mul_nr(fp2_sub(fp2_mul(c1, fp2_add(a.c1, a.c2)), b)), aa);
    const auto t3 = fp2_add(fp2_sub(fp2_mul(c0, fp2_add(a.c0, a.c2)), aa), b);
    const auto t2 = fp2_sub(fp2_sub(fp2_mul(fp2_add(c0, c1), fp2_add(a.c0, a.c1)), aa), b);
    return make_fp6(t1, t2, t3);
}
// fq6.go:295-336
template <int L, int V>
BLSMI_DEV auto fp6_inv(const Fp6<L, V>& a) {
    const Fp2S c0 = fp2_store(fp2_add(fp2_neg(fp2_mul(fp2_mul_nr(a.c2), a.c1)), fp2_sqr(a.c0)));
    const Fp2S c1 = fp2_store(fp2_sub(fp2_mul_nr(fp2_sqr(a.c2)), fp2_mul(a.c0, a.c1)));
    const Fp2S c2 = fp2_store(fp2_sub(fp2_sqr(a.c1), fp2_mul(a.c0, a.c2)));
    auto t = fp2_mul_nr(fp2_add(fp2_mul(a.c2, c1), fp2_mul(a.c1, c2)));
    const Fp2S ti = fp2_store(fp2_inv(fp2_store(fp2_add(t, fp2_mul(a.c0, c0)))));
    return make_fp6(fp2_mul(ti, c0), fp2_mul(ti, c1), fp2_mul(ti, c2));
}
// fq6.go:211-218 with the coefficients (1+u)^((q^P-1)/3), (1+u)^((2q^P-2)/3) of consts.cuh
template <int P, int L, int V>
BLSMI_DEV auto fp6_frob(const Fp6<L, V>& a) {
    return make_fp6(fp2_frob<P>(a.c0), fp2_mul(fp2_frob<P>(a.c1), BLSMI_FP2_K(C_FROB6_C1[P % 6])), fp2_mul(fp2_frob<P>(a.c2), BLSMI_FP2_K(C_FROB6_C2[P % 6])));
}

// ------------------------------------------------------------------------------------------------
// Fq12
// ------------------------------------------------------------------------------------------------
template <int L, int V> BLSMI_DEV Fp12S fp12_store(const Fp12<L, V>& a) { Fp12S r; r.c0 = fp6_store(a.c0); r.c1 = fp6_store(a.c1); return r; }
template <int L, int V> BLSMI_DEV Fp12R fp12_reduced(const Fp12<L, V>& a) { Fp12R r; r.c0 = fp6_reduced(a.c0); r.c1 = fp6_reduced(a.c1); return r; }
template <int L, int V> BLSMI_DEV Fp12W fp12_work(const Fp12<L, V>& a) { Fp12W r; r.c0 = fp6_work(a.c0); r.c1 = fp6_work(a.c1); return r; }
template <int L2, int V2, int L, int V>
BLSMI_DEV Fp12<L2, V2> fp12_relabel(const Fp12<L, V>& a) { Fp12<L2, V2> r; r.c0 = fp6_relabel<L2, V2>(a.c0); r.c1 = fp6_relabel<L2, V2>(a.c1); return r; }
BLSMI_DEV Fp12S fp12_widen(const Fp12W& a) { return fp12_relabel<FpS::L, FpS::V>(a); }       // the working type as the storage type: same limbs, wider promise
BLSMI_DEV Fp12S fp12_one() { Fp12S r; r.c0 = fp6_one(); r.c1 = fp6_zero(); return r; }
template <int L, int V> BLSMI_DEV auto fp12_conj(const Fp12<L, V>& a) { return make_fp12(a.c0, fp6_neg(a.c1)); }   // fq12.go:27-29
// fq12.go:198-213
template <int La, int Va, int Lb, int Vb>
BLSMI_DEV auto fp12_mul(const Fp12<La, Va>& a, const Fp12<Lb, Vb>& b) {
    const auto aa = fp6_norm(fp6_mul(a.c0, b.c0));       // tight bounds (normalised limbs, value bound kept)
    const auto bb = fp6_norm(fp6_mul(a.c1, b.c1));
    const auto t = fp6_mul(fp6_add(a.c1, a.c0), fp6_add(b.c0, b.c1));
    return make_fp12(fp6_add(fp6_mul_nr(bb), aa), fp6_sub(fp6_sub(t, aa), bb));
}
// fq12.go:180-195
template <int L, int V>
BLSMI_DEV auto fp12_sqr(const Fp12<L, V>& a) {
    const auto ab = fp6_norm(fp6_mul(a.c0, a.c1));
    const auto t = fp6_mul(fp6_add(fp6_mul_nr(a.c1), a.c0), fp6_add(a.c0, a.c1));
    return make_fp12(fp6_sub(fp6_sub(t, ab), fp6_mul_nr(ab)), fp6_add(ab, ab));
}
// fq12.go:32-47
template <int L, int V, int L0, int V0, int L1, int V1, int L4, int V4>
BLSMI_DEV auto fp12_mul_by_014(const Fp12<L, V>& a, const Fp2<L0, V0>& c0, const Fp2<L1, V1>& c1, const Fp2<L4, V4>& c4) {
    const auto aa = fp6_norm(fp6_mul_by_01(a.c0, c0, c1));
    const auto bb = fp6_norm(fp6_mul_by_1(a.c1, c4));
    const auto t = fp6_mul_by_01(fp6_add(a.c1, a.c0), c0, fp2_add(c1, c4));
    return make_fp12(fp6_add(fp6_mul_nr(bb), aa), fp6_sub(fp6_sub(t, aa), bb));
}
// fq12.go:216-237
template <int L, int V>
BLSMI_DEV auto fp12_inv(const Fp12<L, V>& a) {
    const Fp6S t = fp6_store(fp6_inv(fp6_store(fp6_sub(fp6_sqr(a.c0), fp6_mul_nr(fp6_store(fp6_sqr(a.c1)))))));
    return make_fp12(fp6_mul(t, a.c0), fp6_neg(fp6_mul(t, a.c1)));
}
// fq12.go:171-177 with (1+u)^((q^P-1)/6)
template <int P, int L, int V>
BLSMI_DEV auto fp12_frob(const Fp12<L, V>& a) {
    const auto c0 = fp6_frob<P>(a.c0);
    const auto c1 = fp6_frob<P>(a.c1);
    const Fp2S k = BLSMI_FP2_K(C_FROB12_C1[P % 12]);
    return make_fp12(c0, make_fp6(fp2_mul(fp2_store(c1.c0), k), fp2_mul(fp2_store(c1.c1), k), fp2_mul(fp2_store(c1.c2), k)));
}
// ---- two sparse line values at once (2-pair Miller loops) ----------------------------------------------------
// A line value is a0 + a1 v + a4 v w (the "014" element above).  The product of two of them,
//   (a0 a0' + xi a4 a4') + (a0 a1' + a1 a0') v + (a1 a1') v^2 + [(a0 a4' + a0' a4) v + (a1 a4' + a1' a4) v^2] w,
// costs 6 Fq2 products by Karatsuba and multiplies into f with 17 (6 + 5 + 6) instead of 13 + 13 for two separate
// sparse multiplications: 23 vs 26 per pair of lines.  Same field element as fq12.go:72-90 applied twice.
struct LinePair { Fp2S l0, l1, l2, l4, l5; };
template <int L0, int V0, int L1, int V1, int L4, int V4, int M0, int W0, int M1, int W1, int M4, int W4>
BLSMI_DEV LinePair line_pair_product(const Fp2<L0, V0>& a0, const Fp2<L1, V1>& a1, const Fp2<L4, V4>& a4,
                                     const Fp2<M0, W0>& b0, const Fp2<M1, W1>& b1, const Fp2<M4, W4>& b4) {
    const auto p00 = fp2_norm(fp2_mul(a0, b0)), p11 = fp2_norm(fp2_mul(a1, b1)), p44 = fp2_norm(fp2_mul(a4, b4));
    LinePair r;
    r.l0 = fp2_store(fp2_add(p00, fp2_mul_nr(p44)));
    r.l1 = fp2_store(fp2_sub(fp2_sub(fp2_mul(fp2_add(a0, a1), fp2_add(b0, b1)), p00), p11));
    r.l2 = fp2_store(p11);
    r.l4 = fp2_store(fp2_sub(fp2_sub(fp2_mul(fp2_add(a0, a4), fp2_add(b0, b4)), p00), p44));
    r.l5 = fp2_store(fp2_sub(fp2_sub(fp2_mul(fp2_add(a1, a4), fp2_add(b1, b4)), p11), p44));
    return r;
}
// (a0 + a1 v + a2 v^2)(b1 v + b2 v^2) = xi (a1 b2 + a2 b1) + (a0 b1 + xi a2 b2) v + (a0 b2 + a1 b1) v^2: five products
template <int L, int V>
BLSMI_DEV auto fp6_mul_by_12(const Fp6<L, V>& a, const Fp2S& b1, const Fp2S& b2) {
    const auto p11 = fp2_norm(fp2_mul(a.c1, b1)), p22 = fp2_norm(fp2_mul(a.c2, b2));
    const auto cross = fp2_sub(fp2_sub(fp2_mul(fp2_add(a.c1, a.c2), fp2_add(b1, b2)), p11), p22);   // a1 b2 + a2 b1
    const auto c0 = fp2_mul_nr(cross);
    const auto c1 = fp2_add(fp2_mul(a.c0, b1), fp2_mul_nr(p22));
    const auto c2 = fp2_add(fp2_mul(a.c0, b2), p11);
    return make_fp6(c0, c1, c2);
}
template <int L, int V>
BLSMI_DEV auto fp12_mul_by_line_pair(const Fp12<L, V>& f, const LinePair& m) {
    const Fp6S m0 = make_fp6(m.l0, m.l1, m.l2);
    const auto t0 = fp6_norm(fp6_mul(f.c0, m0));
    const auto t1 = fp6_norm(fp6_mul_by_12(f.c1, m.l4, m.l5));
    const auto m01 = make_fp6(m.l0, fp2_add(m.l1, m.l4), fp2_add(m.l2, m.l5));
    const auto t2 = fp6_mul(fp6_add(f.c0, f.c1), m01);
    return make_fp12(fp6_add(fp6_mul_nr(t1), t0), fp6_sub(fp6_sub(t2, t0), t1));
}
// Granger-Scott squaring for elements of the cyclotomic subgroup (after the easy part of the final
// exponentiation).  The reference has no such routine -- FQ12.Exp (fq12.go:108-120) squares with a
// full multiplication -- but on the subgroup the value is the same: x^2.
template <class A, class B> struct Pair { A first; B second; };
template <int La, int Va, int Lb, int Vb>
BLSMI_DEV auto fp4_sqr(const Fp2<La, Va>& a, const Fp2<Lb, Vb>& b) {
#if BLSMI_FP4_SQR_BY_PRODUCTS
    // (a + b w)^2 with w^2 = xi:  c1 = 2ab,  c0 = a^2 + xi b^2 = (a + b)(a + xi b) - ab - xi ab
    const auto v = fp2_mul(a, b);
    const auto c0 = fp2_sub(fp2_sub(fp2_mul(fp2_add(a, b), fp2_add(a, fp2_mul_nr(b))), v), fp2_mul_nr(v));
    const auto c1 = fp2_dbl(v);
    return Pair<decltype(c0), decltype(c1)>{c0, c1};
#else
    const auto t0 = fp2_norm(fp2_sqr(a));
    const auto t1 = fp2_norm(fp2_sqr(b));
    const auto c0 = fp2_add(fp2_mul_nr(t1), t0);
    const auto c1 = fp2_sub(fp2_sub(fp2_sqr(fp2_add(a, b)), t0), t1);
    return Pair<decltype(c0), decltype(c1)>{c0, c1};
#endif
}
// outputs are 3t -+ 2z with z an input: the representation doubles per squaring, so each output is
// value-reduced -- the only place in the pairing where a reduction is inherent.  The values travel in the working type (Fp12W: with 28-bit
// limbs the reduced bound those six reductions guarantee), so the Karatsuba sums z + z' and z + xi z' inside fp4_sqr multiply as they are.
BLSMI_DEV Fp12W fp12_cyclotomic_sqr(const Fp12W& f) {
    const Fp2W z0 = f.c0.c0, z4 = f.c0.c1, z3 = f.c0.c2, z2 = f.c1.c0, z1 = f.c1.c1, z5 = f.c1.c2;
    Fp12W r;
    const auto a = fp4_sqr(z0, z1);
    r.c0.c0 = fp2_work(fp2_add(fp2_dbl(fp2_sub(a.first, z0)), a.first));
    r.c1.c1 = fp2_work(fp2_add(fp2_dbl(fp2_add(a.second, z1)), a.second));
    const auto b = fp4_sqr(z2, z3);
    const auto c = fp4_sqr(z4, z5);
    r.c0.c1 = fp2_work(fp2_add(fp2_dbl(fp2_sub(b.first, z4)), b.first));
    r.c1.c2 = fp2_work(fp2_add(fp2_dbl(fp2_add(b.second, z5)), b.second));
    const auto t3n = fp2_mul_nr(c.second);
    r.c1.c0 = fp2_work(fp2_add(fp2_dbl(fp2_add(t3n, z2)), t3n));
    r.c0.c2 = fp2_work(fp2_add(fp2_dbl(fp2_sub(c.first, z3)), c.first));
    return r;
}
// ---- compressed cyclotomic squaring (Karabina): the squaring above maps (z2, z3, z4, z5) to their successors without
// looking at z0, z1, so a run of squarings can carry four coefficients instead of six -- two Fq4 squarings instead of
// three -- and z0, z1 are recovered afterwards from the relation that defines the cyclotomic subgroup:
//   z1 = (xi z5^2 + 3 z4^2 - 2 z3) / (4 z2)        (z1 = 2 z4 z5 / z3 when z2 = 0; 0 for the unit, where z3 = 0 too)
//   z0 = (2 z1^2 + z2 z5 - 3 z3 z4) xi + 1
// F2 is the type the four coefficients travel in: Fp2W for the lane / lane-pair chain, Fp2S where a layout brings its own squaring
// (quad_body.inc) and only recovers z0, z1 here.
template <class F2> struct CycCompressedT { F2 z2, z3, z4, z5; };
using CycCompressed = CycCompressedT<Fp2S>;
using CycCompressedW = CycCompressedT<Fp2W>;
BLSMI_DEV CycCompressedW cyc_compress(const Fp12W& f) {
    CycCompressedW c; c.z4 = f.c0.c1; c.z3 = f.c0.c2; c.z2 = f.c1.c0; c.z5 = f.c1.c2; return c;
}
BLSMI_DEV CycCompressedW cyc_compressed_sqr(const CycCompressedW& g) {
    CycCompressedW r;
    const auto b = fp4_sqr(g.z2, g.z3);
    const auto c = fp4_sqr(g.z4, g.z5);
    r.z4 = fp2_work(fp2_add(fp2_dbl(fp2_sub(b.first, g.z4)), b.first));
    r.z5 = fp2_work(fp2_add(fp2_dbl(fp2_add(b.second, g.z5)), b.second));
    const auto t3n = fp2_mul_nr(c.second);
    r.z2 = fp2_work(fp2_add(fp2_dbl(fp2_add(t3n, g.z2)), t3n));
    r.z3 = fp2_work(fp2_add(fp2_dbl(fp2_sub(c.first, g.z3)), c.first));
    return r;
}
// numerator and denominator of z1 (the denominator is replaced by 1 when both z2 and z3 vanish)
template <class F2>
BLSMI_DEV void cyc_z1_fraction(const CycCompressedT<F2>& g, Fp2S& num, Fp2S& den) {
    const i32 z2zero = fp2_is_zero(g.z2) ? -1 : 0;
    const Fp2S n_reg = fp2_store(fp2_sub(fp2_add(fp2_mul_nr(fp2_sqr(g.z5)), fp2_muls<3>(fp2_sqr(g.z4))), fp2_dbl(g.z3)));
    const Fp2S n_alt = fp2_store(fp2_dbl(fp2_mul(g.z4, g.z5)));
    const Fp2S d_reg = fp2_store(fp2_muls<4>(g.z2));
    num = fp2_select(z2zero, n_alt, n_reg);
    den = fp2_select(z2zero, fp2_relabel<FpS::L, FpS::V>(g.z3), d_reg);
    den = fp2_select(fp2_is_zero(den) ? -1 : 0, fp2_one(), den);
}
template <class F2, int L1, int V1>
BLSMI_DEV Fp12<F2::L, F2::V> cyc_decompress(const CycCompressedT<F2>& g, const Fp2<L1, V1>& z1) {
    const F2 z0 = fp2_as<F2>(fp2_add(fp2_mul_nr(fp2_sub(fp2_add(fp2_dbl(fp2_sqr(z1)), fp2_mul(g.z2, g.z5)), fp2_muls<3>(fp2_mul(g.z3, g.z4)))), fp2_one()));
    Fp12<F2::L, F2::V> r;
    r.c0.c0 = z0; r.c0.c1 = g.z4; r.c0.c2 = g.z3; r.c1.c0 = g.z2; r.c1.c1 = fp2_as<F2>(z1); r.c1.c2 = g.z5;
    return r;
}
template <int La, int Va, int Lb, int Vb>
BLSMI_DEV bool fp12_eq(const Fp12<La, Va>& a, const Fp12<Lb, Vb>& b) {
    bool e = true;
    e &= fp2_eq(a.c0.c0, b.c0.c0); e &= fp2_eq(a.c0.c1, b.c0.c1); e &= fp2_eq(a.c0.c2, b.c0.c2);
    e &= fp2_eq(a.c1.c0, b.c1.c0); e &= fp2_eq(a.c1.c1, b.c1.c1); e &= fp2_eq(a.c1.c2, b.c1.c2);
    return e;
}

