// fp2_single.inc -- Fq2 with both coefficients in one lane (the layout of every kernel except the
// lane-pair pairing kernels).  Included inside a namespace by tower.cuh; the Fq6/Fq12 code of
// tower_body.inc is written against exactly this interface (see fp2_pair.inc for the other layout).
template <int La, int Va, int Lb, int Vb>
BLSMI_DEV auto make_fp2(const Fp<La, Va>& a, const Fp<Lb, Vb>& b) {
    constexpr int L = imax(La, Lb), V = imax(Va, Vb);
    Fp2<L, V> r;
    r.c0 = fp_relabel<L, V>(a);
    r.c1 = fp_relabel<L, V>(b);
    return r;
}
template <int L2, int V2, int L, int V>
BLSMI_DEV Fp2<L2, V2> fp2_relabel(const Fp2<L, V>& a) {
    Fp2<L2, V2> r;
    r.c0 = fp_relabel<L2, V2>(a.c0);
    r.c1 = fp_relabel<L2, V2>(a.c1);
    return r;
}
// ------------------------------------------------------------------------------------------------
// Fq2
// ------------------------------------------------------------------------------------------------
template <int La, int Va, int Lb, int Vb> BLSMI_DEV auto fp2_add(const Fp2<La, Va>& a, const Fp2<Lb, Vb>& b) { return make_fp2(fp_add(a.c0, b.c0), fp_add(a.c1, b.c1)); }
template <int La, int Va, int Lb, int Vb> BLSMI_DEV auto fp2_sub(const Fp2<La, Va>& a, const Fp2<Lb, Vb>& b) { return make_fp2(fp_sub(a.c0, b.c0), fp_sub(a.c1, b.c1)); }
template <int L, int V> BLSMI_DEV auto fp2_neg(const Fp2<L, V>& a) { return make_fp2(fp_neg(a.c0), fp_neg(a.c1)); }
template <int L, int V> BLSMI_DEV auto fp2_dbl(const Fp2<L, V>& a) { return make_fp2(fp_dbl(a.c0), fp_dbl(a.c1)); }
template <int K, int L, int V> BLSMI_DEV auto fp2_muls(const Fp2<L, V>& a) { return make_fp2(fp_muls<K>(a.c0), fp_muls<K>(a.c1)); }
template <int L, int V> BLSMI_DEV auto fp2_conj(const Fp2<L, V>& a) { return make_fp2(a.c0, fp_neg(a.c1)); }
template <int L, int V> BLSMI_DEV auto fp2_norm(const Fp2<L, V>& a) { return make_fp2(fp_norm(a.c0), fp_norm(a.c1)); }
template <int L, int V> BLSMI_DEV Fp2S fp2_store(const Fp2<L, V>& a) { Fp2S r; r.c0 = fp_store(a.c0); r.c1 = fp_store(a.c1); return r; }
template <int L, int V> BLSMI_DEV Fp2R fp2_reduced(const Fp2<L, V>& a) { Fp2R r; r.c0 = fp_reduced(a.c0); r.c1 = fp_reduced(a.c1); return r; }
template <int L, int V> BLSMI_DEV bool fp2_is_zero(const Fp2<L, V>& a) { return fp_is_zero(a.c0) & fp_is_zero(a.c1); }
template <int La, int Va, int Lb, int Vb> BLSMI_DEV bool fp2_eq(const Fp2<La, Va>& a, const Fp2<Lb, Vb>& b) { return fp2_is_zero(fp2_sub(a, b)); }
template <int L, int V> BLSMI_DEV Fp2<L, V> fp2_select(i32 m, const Fp2<L, V>& a, const Fp2<L, V>& b) { Fp2<L, V> r; r.c0 = fp_select(m, a.c0, b.c0); r.c1 = fp_select(m, a.c1, b.c1); return r; }
BLSMI_DEV Fp2S fp2_zero() { Fp2S r; r.c0 = fp_zero(); r.c1 = fp_zero(); return r; }
BLSMI_DEV Fp2S fp2_one() { Fp2S r; r.c0 = fp_one(); r.c1 = fp_zero(); return r; }

// fq2.go:41-45: multiply by the non-residue 1+u
template <int L, int V> BLSMI_DEV auto fp2_mul_nr(const Fp2<L, V>& a) { return make_fp2(fp_sub(a.c0, a.c1), fp_add(a.c0, a.c1)); }
// fq2.go:116-130 (Karatsuba, 3 Fq multiplications)
template <int La, int Va, int Lb, int Vb>
BLSMI_DEV auto fp2_mul(const Fp2<La, Va>& a, const Fp2<Lb, Vb>& b) {
    const auto aa = fp_mul(a.c0, b.c0);
    const auto bb = fp_mul(a.c1, b.c1);
    const auto t = fp_mul(fp_add(a.c0, a.c1), fp_add(b.c0, b.c1));
    return make_fp2(fp_sub(aa, bb), fp_sub(fp_sub(t, aa), bb));
}
// fq2.go:75-89 (complex squaring, 2 Fq multiplications)
template <int L, int V>
BLSMI_DEV auto fp2_sqr(const Fp2<L, V>& a) {
    const auto ab = fp_mul(a.c0, a.c1);
    const auto c0 = fp_mul(fp_add(a.c0, a.c1), fp_sub(a.c0, a.c1));
    return make_fp2(c0, fp_dbl(ab));
}
template <int La, int Va, int Lb, int Vb>
BLSMI_DEV auto fp2_mul_fp(const Fp2<La, Va>& a, const Fp<Lb, Vb>& s) { return make_fp2(fp_mul(a.c0, s), fp_mul(a.c1, s)); }
// fq2.go:133-147
template <int L, int V>
BLSMI_DEV auto fp2_inv(const Fp2<L, V>& a) {
    const FpS t = fp_inv(fp_add(fp_sqr(a.c0), fp_sqr(a.c1)));
    return make_fp2(fp_mul(a.c0, t), fp_neg(fp_mul(a.c1, t)));
}
// fq2.go:156-158: c1 *= (-1)^power
template <int P, int L, int V>
BLSMI_DEV auto fp2_frob(const Fp2<L, V>& a) {
    if constexpr (P % 2 == 0) return a; else return fp2_conj(a);
}

// fq2.go:177-193: exponentiation by a fixed public exponent, bits MSB-first from constant memory
template <int L, int V>
BLSMI_DEV Fp2S fp2_pow_const(const Fp2<L, V>& a, const u32* ebits, int nbits) {
    const Fp2S base = fp2_store(a);
    Fp2S res = base;
    for (int i = nbits - 2; i >= 0; i--) {
        res = fp2_store(fp2_sqr(res));
        if ((ebits[i >> 5] >> (i & 31)) & 1) res = fp2_store(fp2_mul(res, base));
    }
    return res;
}
// fq2.go:198-232 (Algorithm 9 of eprint 2012/685), evaluated without divergent control flow:
// both tails are computed and the result is selected.
template <int L, int V>
BLSMI_DEV Fp2S fp2_sqrt(const Fp2<L, V>& a_in, bool& ok) {
    const Fp2S a = fp2_store(a_in);
    const bool zero = fp2_is_zero(a);
    const Fp2S a1 = fp2_pow_const(a, C_QM3O4, BLSMI_QM3O4_BITS);
    const Fp2S alpha = fp2_store(fp2_mul(fp2_sqr(a1), a));
    const Fp2S a0 = fp2_store(fp2_mul(fp2_conj(alpha), alpha));
    Fp2S neg1; neg1.c0 = C_NEGONE; neg1.c1 = fp_zero();
    const bool nonres = fp2_eq(a0, neg1);
    const Fp2S x0 = fp2_store(fp2_mul(a1, a));
    const bool alpha_m1 = fp2_eq(alpha, neg1);
    Fp2S xu; xu.c0 = fp_store(fp_neg(x0.c1)); xu.c1 = x0.c0;              // x0 * u
    const Fp2S b = fp2_pow_const(fp2_add(alpha, fp2_one()), C_QM1O2, BLSMI_QM1O2_BITS);
    const Fp2S xb = fp2_store(fp2_mul(b, x0));
    Fp2S r = fp2_select(alpha_m1 ? -1 : 0, xu, xb);
    r = fp2_select(zero ? -1 : 0, fp2_zero(), r);
    ok = zero | !nonres;
    return r;
}

// A square root of a (either one) from two Fq exponentiations instead of two Fq2 exponentiations (~2.4x fewer
// Fq multiplications than the routine above).  Every caller on the verify path normalises the sign of the root
// afterwards (g2.go:983-988, 1021-1026 sign(y) := sign(t); g2.go:149-169 and :1074-1077 pick y or -y by
// comparison), so which of the two roots comes back is immaterial and the outputs stay bit-identical.
//   n = a0^2 + a1^2 is a square in Fq  <=>  a is a square in Fq2;  s = sqrt(n)
//   d = (a0 + s)/2;  f = d^((q-3)/4), r = f d  =>  r^2 = +-d  and  1/r = +-f
//   r^2 =  d:  root = (r, a1 f/2);      r^2 = -d:  root = (-a1 f/2, r)
// (d = 0 happens only for a = a0 a non-residue of Fq: take d = a0 instead, i.e. the other sign of s.)
// step 1: n = N(a), s = n^((q+1)/4); residue <=> s^2 == n (otherwise s^2 == -n)
template <int WAVE = 0>
BLSMI_DEV FpS fp2_norm_root(const Fp2S& a, FpS& n, bool& ok) {
    n = fp_store(fp_add(fp_sqr(a.c0), fp_sqr(a.c1)));
    FpS e;
    if constexpr (WAVE != 0) e = fp_pow_spread<WAVE>(n, C_QM3O4, BLSMI_QM3O4_BITS);
    else e = fp_pow_qm3o4(n);
    const FpS s = fp_store(fp_mul(e, n));
    ok = fp_eq(fp_sqr(s), n);
    return s;
}
// step 2: a root of a given s with s^2 == N(a)
// WAVE: the wave works on one wave-uniform a; the exponentiation runs with one limb per lane (fp_row.cuh)
template <int WAVE = 0>
BLSMI_DEV Fp2S fp2_sqrt_from_norm_root(const Fp2S& a, const FpS& s) {
    FpS d = fp_store(fp_mul(fp_add(a.c0, s), C_HALF));
    d = fp_select(fp_is_zero(d) ? -1 : 0, a.c0, d);
    FpS f;
    if constexpr (WAVE != 0) f = fp_pow_spread<WAVE>(d, C_QM3O4, BLSMI_QM3O4_BITS);
    else f = fp_pow_qm3o4(d);
    const FpS r = fp_store(fp_mul(f, d));
    const FpS h = fp_store(fp_mul(fp_mul(a.c1, f), C_HALF));
    const i32 plus = fp_eq(fp_sqr(r), d) ? -1 : 0;
    Fp2S x;
    x.c0 = fp_select(plus, r, fp_store(fp_neg(h)));
    x.c1 = fp_select(plus, h, r);
    return x;
}
template <int WAVE = 0, int L, int V>
BLSMI_DEV Fp2S fp2_sqrt_any(const Fp2<L, V>& a_in, bool& ok) {
    const Fp2S a = fp2_store(a_in);
    FpS n;
    const FpS s = fp2_norm_root<WAVE>(a, n, ok);
    return fp2_sqrt_from_norm_root<WAVE>(a, s);
}

// table of Fq2 values shared by all lanes: entry e = [c0 limbs][c1 limbs]
BLSMI_DEV Fp2S fp2_table_load(const i32* t, int e) {
    Fp2S r;
#pragma unroll
    for (int i = 0; i < NL; i++) { r.c0.v[i] = t[(2 * e) * NL + i]; r.c1.v[i] = t[(2 * e + 1) * NL + i]; }
    return r;
}
BLSMI_DEV void fp2_table_store(i32* t, int e, const Fp2S& a) {
#pragma unroll
    for (int i = 0; i < NL; i++) { t[(2 * e) * NL + i] = a.c0.v[i]; t[(2 * e + 1) * NL + i] = a.c1.v[i]; }
}

// constants of consts.cuh are stored in this layout already
#undef BLSMI_FP2_K
#define BLSMI_FP2_K(x) (x)
#undef BLSMI_FP4_SQR_BY_PRODUCTS
#define BLSMI_FP4_SQR_BY_PRODUCTS 0     // here a square is 2 and a product 3 Fq multiplications: three squares win
