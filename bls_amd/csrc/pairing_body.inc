// pairing_body.inc -- Miller loop and final exponentiation over the Fq2 layer of the including namespace
// (single-lane layout in blsmi::, lane-pair layout in blsmi::pairl::).  See pairing.cuh.

struct G2Proj { Fp2S x, y, z; };

// Out-of-line Fq12 operations on references: between calls the 180-word operands live in the
// lane's scratch (a few hundred dword accesses against >10^4 VALU instructions per call), inside a
// call everything is in registers.  One copy of each body serves every kernel, which keeps each
// body's register allocation tractable and the code small.
// The operands and results are of the working type (tower_body.inc: Fp12W -- with 28-bit limbs every coefficient carries the reduced bound
// its last value reduction left, so each coefficient is reduced once per operation, on the way out, and never again as an operand).
BLSMI_NOINLINE void nf_fp12_mul(Fp12W& r, const Fp12W& a, const Fp12W& b) { r = fp12_work(fp12_mul(a, b)); }
BLSMI_NOINLINE void nf_fp12_sqr(Fp12W& r, const Fp12W& a) { r = fp12_work(fp12_sqr(a)); }
BLSMI_NOINLINE void nf_fp12_cyc_sqr(Fp12W& r, const Fp12W& a) { r = fp12_cyclotomic_sqr(a); }
BLSMI_NOINLINE void nf_fp12_inv(Fp12W& r, const Fp12W& a) { r = fp12_work(fp12_inv(a)); }
BLSMI_NOINLINE void nf_fp12_frob1(Fp12W& r, const Fp12W& a) { r = fp12_work(fp12_frob<1>(a)); }
BLSMI_NOINLINE void nf_fp12_frob2(Fp12W& r, const Fp12W& a) { r = fp12_work(fp12_frob<2>(a)); }
BLSMI_NOINLINE void nf_fp12_frob3(Fp12W& r, const Fp12W& a) { r = fp12_work(fp12_frob<3>(a)); }
BLSMI_DEV void fp12_conj_inplace(Fp12W& a) { a.c1 = fp6_work(fp6_neg(a.c1)); }

// g2.go:655-708
BLSMI_NOINLINE void doubling_step(G2Proj& r, Fp2S& o0, Fp2S& o1, Fp2S& o2) {
    const auto tmp0 = fp2_norm(fp2_sqr(r.x));
    const auto tmp1 = fp2_norm(fp2_sqr(r.y));
    const auto tmp2 = fp2_norm(fp2_sqr(tmp1));
    const auto tmp3 = fp2_norm(fp2_dbl(fp2_sub(fp2_sub(fp2_sqr(fp2_add(tmp1, r.x)), tmp0), tmp2)));
    const auto tmp4 = fp2_norm(fp2_muls<3>(tmp0));
    const auto tmp6 = fp2_norm(fp2_add(r.x, tmp4));
    const auto tmp5 = fp2_norm(fp2_sqr(tmp4));
    const auto zsq = fp2_norm(fp2_sqr(r.z));
    const auto nx = fp2_norm(fp2_sub(fp2_sub(tmp5, tmp3), tmp3));
    const auto nz = fp2_norm(fp2_sub(fp2_sub(fp2_sqr(fp2_add(r.z, r.y)), tmp1), zsq));
    const auto ny = fp2_norm(fp2_sub(fp2_mul(fp2_sub(tmp3, nx), tmp4), fp2_muls<8>(tmp2)));
    o1 = fp2_store(fp2_neg(fp2_dbl(fp2_mul(tmp4, zsq))));
    o2 = fp2_store(fp2_sub(fp2_sub(fp2_sub(fp2_sqr(tmp6), tmp0), tmp5), fp2_muls<4>(tmp1)));
    o0 = fp2_store(fp2_dbl(fp2_mul(nz, zsq)));
    r.x = fp2_store(nx); r.y = fp2_store(ny); r.z = fp2_store(nz);
}
// g2.go:710-772
BLSMI_NOINLINE void addition_step(G2Proj& r, const Fp2S& qx, const Fp2S& qy, Fp2S& o0, Fp2S& o1, Fp2S& o2) {
    const auto zsq = fp2_norm(fp2_sqr(r.z));
    const auto ysq = fp2_norm(fp2_sqr(qy));
    const auto t0 = fp2_norm(fp2_mul(zsq, qx));
    const auto t1 = fp2_norm(fp2_mul(fp2_sub(fp2_sub(fp2_sqr(fp2_add(qy, r.z)), ysq), zsq), zsq));
    const auto t2 = fp2_norm(fp2_sub(t0, r.x));
    const auto t3 = fp2_norm(fp2_sqr(t2));
    const auto t4 = fp2_norm(fp2_muls<4>(t3));
    const auto t5 = fp2_norm(fp2_mul(t4, t2));
    const auto t6 = fp2_norm(fp2_sub(fp2_sub(t1, r.y), r.y));
    const auto t9 = fp2_norm(fp2_mul(t6, qx));
    const auto t7 = fp2_norm(fp2_mul(t4, r.x));
    const auto nx = fp2_norm(fp2_sub(fp2_sub(fp2_sub(fp2_sqr(t6), t5), t7), t7));
    const auto nz = fp2_norm(fp2_sub(fp2_sub(fp2_sqr(fp2_add(r.z, t2)), zsq), t3));
    const auto t8 = fp2_norm(fp2_mul(fp2_sub(t7, nx), t6));
    const auto ny = fp2_norm(fp2_sub(t8, fp2_dbl(fp2_mul(r.y, t5))));
    const auto t10 = fp2_norm(fp2_sub(fp2_sub(fp2_sqr(fp2_add(qy, nz)), ysq), fp2_sqr(nz)));
    o2 = fp2_store(fp2_sub(fp2_dbl(t9), t10));
    o0 = fp2_store(fp2_dbl(nz));
    o1 = fp2_store(fp2_dbl(fp2_neg(t6)));
    r.x = fp2_store(nx); r.y = fp2_store(ny); r.z = fp2_store(nz);
}
// Homogeneous projective steps on E' (y^2 = x^3 + b', b' = 4 xi): 4 multiplications + 5 squarings per doubling against the
// 3 + 8 of the reference's step above, same (o0, o1, o2) interface.  The lines differ from the reference's by factors in
// Fq2*, which the final exponentiation removes: used wherever only FinalExponentiation(MillerLoop) leaves the device
// (Pairing, the verify family); the exported MillerLoop keeps the reference's steps.  Same formulas as gen_lat.py:
//   A = XY, B = Y^2, E = 3 b' Z^2 = 12 xi Z^2, H = 2YZ, F = 3E, G = B + F
//   X3 = 2 A (B - F),  Y3 = G^2 - 12 E^2,  Z3 = 4 B H          line: (B - E) + (-3 X^2) xP v + H yP v w
BLSMI_DEV void doubling_step_h_i(G2Proj& r, Fp2S& o0, Fp2S& o1, Fp2S& o2) {
    const auto A = fp2_norm(fp2_mul(r.x, r.y));
    const auto B = fp2_norm(fp2_sqr(r.y));
    const auto X2 = fp2_norm(fp2_sqr(r.x));
    const auto H = fp2_norm(fp2_dbl(fp2_mul(r.y, r.z)));
    // E is trimmed where it is made (28-bit limbs: value-reduced, 72 -> 5 half-q): G = B + 3E and E then square as they are and B - E stores
    // without a reduction -- two reductions a step (E, Y3) instead of four (G and E before their squares, Y3, B - E).  The running point
    // itself gains nothing from the reduced type: X, Y, Z multiply in one pass under the storage bound already.
    const auto E = fp2_trim(fp2_muls<12>(fp2_norm(fp2_mul_nr(fp2_norm(fp2_sqr(r.z))))));
    const auto F = fp2_norm(fp2_muls<3>(E));
    const auto G = fp2_norm(fp2_add(B, F));
    const auto nx = fp2_norm(fp2_dbl(fp2_mul(A, fp2_norm(fp2_sub(B, F)))));
    const auto ny = fp2_norm(fp2_sub(fp2_sqr(G), fp2_muls<12>(fp2_norm(fp2_sqr(E)))));
    const auto nz = fp2_norm(fp2_muls<4>(fp2_norm(fp2_mul(B, H))));
    o2 = fp2_store(fp2_sub(B, E));
    o1 = fp2_store(fp2_neg(fp2_muls<3>(X2)));
    o0 = fp2_store(H);
    r.x = fp2_store(nx); r.y = fp2_store(ny); r.z = fp2_store(nz);
}
BLSMI_NOINLINE void doubling_step_h(G2Proj& r, Fp2S& o0, Fp2S& o1, Fp2S& o2) { doubling_step_h_i(r, o0, o1, o2); }
// mixed addition R + Q and the chord:  th = Y - yq Z, la = X - xq Z, C = th^2, D = la^2, E = la D, F = Z C, G = X D, Hh = E + F - 2G
//   X3 = la Hh,  Y3 = th (G - Hh) - E Y,  Z3 = Z E          line: (th xq - la yq) + (-th) xP v + la yP v w
BLSMI_NOINLINE void addition_step_h(G2Proj& r, const Fp2S& qx, const Fp2S& qy, Fp2S& o0, Fp2S& o1, Fp2S& o2) {
    const auto th = fp2_norm(fp2_sub(r.y, fp2_mul(qy, r.z)));
    const auto la = fp2_norm(fp2_sub(r.x, fp2_mul(qx, r.z)));
    const auto C = fp2_norm(fp2_sqr(th));
    const auto D = fp2_norm(fp2_sqr(la));
    const auto E = fp2_norm(fp2_mul(la, D));
    const auto F = fp2_norm(fp2_mul(r.z, C));
    const auto G = fp2_norm(fp2_mul(r.x, D));
    const auto Hh = fp2_norm(fp2_sub(fp2_add(E, F), fp2_dbl(G)));
    const auto nx = fp2_norm(fp2_mul(la, Hh));
    const auto ny = fp2_norm(fp2_sub(fp2_mul(th, fp2_norm(fp2_sub(G, Hh))), fp2_mul(E, r.y)));
    const auto nz = fp2_norm(fp2_mul(r.z, E));
    o2 = fp2_store(fp2_sub(fp2_mul(th, qx), fp2_mul(la, qy)));
    o1 = fp2_store(fp2_neg(th));
    o0 = fp2_store(la);
    r.x = fp2_store(nx); r.y = fp2_store(ny); r.z = fp2_store(nz);
}
template <bool EXACT> BLSMI_DEV void dbl_step(G2Proj& r, Fp2S& o0, Fp2S& o1, Fp2S& o2) {
    // Inlining the homogeneous step into the loops (the running point would stay in registers instead of crossing a call boundary
    // 63 times) was measured and is NOT a gain here -- k_miller1h_pair 9.65 ms against 9.5 ms per 65 536 -- unlike in the G1 / G2
    // ladders of k_curve.hip: the accumulator f does not fit beside it.
    if constexpr (EXACT) doubling_step(r, o0, o1, o2); else doubling_step_h(r, o0, o1, o2);
}
template <bool EXACT> BLSMI_DEV void add_step(G2Proj& r, const Fp2S& qx, const Fp2S& qy, Fp2S& o0, Fp2S& o1, Fp2S& o2) {
    if constexpr (EXACT) addition_step(r, qx, qy, o0, o1, o2); else addition_step_h(r, qx, qy, o0, o1, o2);
}
// pairing.go:28-39: f *= line evaluated at P (sparse 014 multiplication)
BLSMI_NOINLINE void ell(Fp12W& f, const Fp2S& o0, const Fp2S& o1, const Fp2S& o2, const FpS& px, const FpS& py) {
    const auto c0 = fp2_mul_fp(o0, py);
    const auto c1 = fp2_mul_fp(o1, px);
    // f enters the product under the storage bound on purpose: read as reduced it saves one operand reduction (13 multiply-adds) and
    // the body then spills 416 instead of 240 bytes a lane (200 against 118 scratch accesses), which every Miller kernel's frame inherits.
    // Six calls a loop; ell_sqr, at 62, is where the reduced operand pays.
    f = fp12_work(fp12_mul_by_014(fp12_widen(f), o2, c1, c0));
}

// f = (f * line(P))^2 in one call: the 180-word accumulator crosses the call boundary once per iteration.  (Expanded in line at the loop's
// one call site, so that f would be a local of the kernel, it was measured slower: k_miller1h_pair 9.83 against 9.31 ms -- the kernel
// then spills 3 072 instead of 1 664 bytes a lane.)
BLSMI_NOINLINE void ell_sqr(Fp12W& f, const Fp2S& o0, const Fp2S& o1, const Fp2S& o2, const FpS& px, const FpS& py) {
    const auto c0 = fp2_mul_fp(o0, py);
    const auto c1 = fp2_mul_fp(o1, px);
    const Fp12W g = fp12_work(fp12_mul_by_014(f, o2, c1, c0));
    f = fp12_work(fp12_sqr(g));
}

// two lines (one per pair of a 2-pair loop) multiplied into f as one 5-coefficient element; SQR: followed by f^2
template <bool SQR>
BLSMI_NOINLINE void ell2(Fp12W& f, const Fp2S& a0, const Fp2S& a1, const Fp2S& a2, const FpS& ax, const FpS& ay,
                         const Fp2S& b0, const Fp2S& b1, const Fp2S& b2, const FpS& bx, const FpS& by) {
    // line value of (o0, o1, o2) at P: o2 + (o1 P.x) v + (o0 P.y) v w   (pairing.go:28-39)
    const LinePair m = line_pair_product(a2, fp2_mul_fp(a1, ax), fp2_mul_fp(a0, ay), b2, fp2_mul_fp(b1, bx), fp2_mul_fp(b0, by));
    const Fp12W g = fp12_work(fp12_mul_by_line_pair(f, m));
    if (SQR) f = fp12_work(fp12_sqr(g)); else f = g;
}

// The walk over the bits of |x| >> 1 below its leading one (pairing.go:41-70; g2.go:650-801 runs the same walk to prepare a point),
// written ONCE for the single-lane, lane-pair and lane-quad loops: a doubling per bit; where the bit is set the line(s) go into f and an
// addition follows; multiply-and-square; after the last bit one more doubling, whose line(s) go in unsquared.  The caller sets f to one
// before and conjugates after (blsIsNegative, pairing.go:71-73).  (The lane-row loops keep a shape of their own, written out: row_body.inc.)
// `tick(done)` runs at the top of every bit with the number of bits already walked (0..61): wave-uniform, the loop index lives in a scalar
// register (miller_loop<.., YIELD> lowers the wave's priority there; everyone else passes nothing).
struct NoTick { BLSMI_DEV void operator()(int) const {} };
template <class Dbl, class Add, class Mul, class MulSqr, class Tick = NoTick>
BLSMI_DEV void x_bit_walk(Dbl dbl, Add add, Mul mul, MulSqr mul_sqr, Tick tick = Tick()) {
    const u64 xr = BLSMI_X_ABS >> 1;
    for (int i = 61; i >= 0; i--) {
        tick(61 - i);
        dbl();
        if ((xr >> i) & 1) { mul(); add(); }
        mul_sqr();
    }
    dbl();
    mul();
}

// pairing.go:16-75 for one pair, or for two pairs sharing the squarings.
// PRE0: the G2 point of pair 0 is the fixed generator, whose 68 line-coefficient triples (the reference's
// G2Prepared, g2.go:639-801) were computed once at start-up by the same doubling/addition steps and are read
// from `pre` ([line][coefficient][c0|c1][limb]) instead of being recomputed per tuple.
BLSMI_DEV void load_line(const i32* pre, int line, Fp2S& o0, Fp2S& o1, Fp2S& o2) {
    o0 = fp2_table_load(pre, 3 * line); o1 = fp2_table_load(pre, 3 * line + 1); o2 = fp2_table_load(pre, 3 * line + 2);
}
BLSMI_DEV void store_line(i32* table, int line, const Fp2S& o0, const Fp2S& o1, const Fp2S& o2) {
    fp2_table_store(table, 3 * line, o0); fp2_table_store(table, 3 * line + 1, o1); fp2_table_store(table, 3 * line + 2, o2);
}
// EXACT: the reference's doubling / addition steps -- f is then the reference's Miller value itself; otherwise the
// homogeneous steps, f differs by a factor the final exponentiation removes.
// PRE1 (two-pair loops): pair 1's lines come from a table as well -- `pre1`, like `pre`, may differ from lane pair to lane pair
// (the prepared public keys of blsmi_g2_prepare_batch_dev, one 24 KB table per key); q[k] of a prepared pair is not read.
// The running point of the LAST pair in LDS (lds_r: 45 words x the workgroup's 64 lanes, word-major; lane-pair kernels with the
// homogeneous steps only): the doubling step then runs IN LINE in the loop, with the point fetched from and put back to LDS around it,
// instead of out of line on a reference into the lane's scratch -- a round trip through scratch costs ~3 400 cycles under load, LDS ~100
// (DESIGN 7; tools/ubench_core.hip: 64.6 k cycles per step against 77-81 k).  The point cannot simply stay in registers: the out-of-line
// ell_sqr / ell2 between two steps takes the whole register file.
BLSMI_DEV void lds_put_proj(i32* l, const G2Proj& r) {
    const FpS* c = reinterpret_cast<const FpS*>(&r);
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
        for (int i = 0; i < NL; i++) l[(j * NL + i) * 64 + threadIdx.x] = c[j].v[i];
}
BLSMI_DEV G2Proj lds_get_proj(const i32* l) {
    G2Proj r;
    FpS* c = reinterpret_cast<FpS*>(&r);
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
        for (int i = 0; i < NL; i++) c[j].v[i] = l[(j * NL + i) * 64 + threadIdx.x];
    return r;
}
// YIELD > 0 (the lane-pair kernels that run two waves per SIMD, pair_kernels.inc): the wave entered at s_setprio 1 and goes down to 0 once
// YIELD bits are walked, so that the wave it shares the SIMD with -- still at 1 if it is behind -- catches up.
template <int NP, bool PRE0 = false, bool EXACT = true, bool PRE1 = false, int YIELD = 0, class G1P, class G2P>
BLSMI_DEV void miller_loop(Fp12S& out, const G1P (&p)[NP], const G2P (&q)[NP], const i32* pre = nullptr, const i32* pre1 = nullptr, i32* lds_r = nullptr) {
    static_assert(NP == 1 || NP == 2, "one pair, or two pairs sharing the squarings");
    constexpr int LAST = NP - 1;
    constexpr bool PRE_LAST = NP == 1 ? PRE0 : PRE1;                       // the last pair's lines come from a table: it has no running point
    G2Proj r[NP];
#pragma unroll
    for (int k = 0; k < NP; k++) { r[k].x = q[k].x; r[k].y = q[k].y; r[k].z = fp2_one(); }
    Fp12W f = fp12_work(fp12_one());                                   // the accumulator, in the working type from the first line to the last
    const bool in_lds = !EXACT && !PRE_LAST && lds_r != nullptr;           // the last pair's running point in LDS, its doubling step in line (see lds_put_proj)
    if (in_lds) lds_put_proj(lds_r, r[LAST]);
    auto dbl_last = [&](Fp2S& a0, Fp2S& a1, Fp2S& a2) {
        if (in_lds) { G2Proj t = lds_get_proj(lds_r); doubling_step_h_i(t, a0, a1, a2); lds_put_proj(lds_r, t); }
        else dbl_step<EXACT>(r[LAST], a0, a1, a2);
    };
    auto add_last = [&](Fp2S& a0, Fp2S& a1, Fp2S& a2) {
        if (in_lds) { G2Proj t = lds_get_proj(lds_r); add_step<EXACT>(t, q[LAST].x, q[LAST].y, a0, a1, a2); lds_put_proj(lds_r, t); }
        else add_step<EXACT>(r[LAST], q[LAST].x, q[LAST].y, a0, a1, a2);
    };
    Fp2S o0, o1, o2;
    int line = 0;
    auto tick = [](int done) {
        if constexpr (YIELD > 0) { if (done == YIELD) pair_yield_drop(); }
        else (void)done;
    };
    if constexpr (NP == 1) {
        x_bit_walk([&] { if (PRE0) load_line(pre, line++, o0, o1, o2); else dbl_last(o0, o1, o2); },
                   [&] { if (PRE0) load_line(pre, line++, o0, o1, o2); else add_last(o0, o1, o2); },
                   [&] { ell(f, o0, o1, o2, p[0].x, p[0].y); },
                   [&] { ell_sqr(f, o0, o1, o2, p[0].x, p[0].y); }, tick);
    } else {
        // both pairs' lines of a step are multiplied together first (ell2): 23 instead of 26 Fq2 products per step
        Fp2S n0, n1, n2;
        int line1 = 0;
        x_bit_walk([&] { if (PRE0) load_line(pre, line++, o0, o1, o2); else dbl_step<EXACT>(r[0], o0, o1, o2);
                         if (PRE1) load_line(pre1, line1++, n0, n1, n2); else dbl_last(n0, n1, n2); },
                   [&] { if (PRE0) load_line(pre, line++, o0, o1, o2); else add_step<EXACT>(r[0], q[0].x, q[0].y, o0, o1, o2);
                         if (PRE1) load_line(pre1, line1++, n0, n1, n2); else add_last(n0, n1, n2); },
                   [&] { ell2<false>(f, o0, o1, o2, p[0].x, p[0].y, n0, n1, n2, p[1].x, p[1].y); },
                   [&] { ell2<true>(f, o0, o1, o2, p[0].x, p[0].y, n0, n1, n2, p[1].x, p[1].y); }, tick);
    }
    fp12_conj_inplace(f);                                              // blsIsNegative (pairing.go:71-73)
    out = fp12_widen(f);
}
// the 68 triples of one G2 point, in loop order, written by every lane that calls it (identical values)
BLSMI_DEV void prepare_lines(const Fp2S& qx, const Fp2S& qy, i32* table) {
    G2Proj r; r.x = qx; r.y = qy; r.z = fp2_one();
    Fp2S o0, o1, o2;
    int line = 0;
    x_bit_walk([&] { doubling_step(r, o0, o1, o2); store_line(table, line++, o0, o1, o2); },
               [&] { addition_step(r, qx, qy, o0, o1, o2); store_line(table, line++, o0, o1, o2); },
               [] {}, [] {});                                             // no accumulator: the lines are the result
}

// ---- final exponentiation, written ONCE for every lane layout over a struct O of static operations on the layout's Fq12 type O::T
// (Fp12Ops below; QuadOps in quad_body.inc, RowOps in row_body.inc).  Every operation is one call into the layout's own routine and writes
// its first argument, which may be one of its operands.
//
// pairing.go:92-98 (ExpByX): f^|e| then conjugate.  f must lie in the cyclotomic subgroup.
// Square-and-multiply from the top bit, as the reference does.  A run of >= O::MIN_RUN squarings with no
// multiplication in between (|x| has runs of 32 and 16) is walked in Karabina's compressed form -- four coefficients, two
// Fq4 squarings per step instead of three -- and decompressed once at its end (one safegcd inversion): same element.
// O::x_sqr is one plain squaring inside this loop, O::x_sqr_run a compressed run; MIN_RUN = 0: the layout never compresses (and has no
// x_sqr_run).  (x_sqr, x_sqr_run and exp_x are named apart from the layouts' routines cyc_sqr_run / exp_by_x, which a member would hide.)
template <class O>
BLSMI_DEV void exp_by_x_loop(typename O::T& out, const typename O::T& f, u64 e) {
    typename O::T res = f;
    int i = 62 - __builtin_clzll(e);                                       // next bit to process
    while (i >= 0) {
        // squarings up to and including the next set bit (or down to bit 0)
        const u64 below = e & ((2ull << i) - 1);                           // bits i..0
        const int next = below ? 63 - __builtin_clzll(below) : -1;         // position of the next set bit at or below i
        const int run = next < 0 ? i + 1 : i - next + 1;                   // squarings up to and including that bit
        bool plain = true;
        if constexpr (O::MIN_RUN > 0)
            if (run >= O::MIN_RUN) { O::x_sqr_run(res, res, run); plain = false; }
        if (plain) for (int j = 0; j < run; j++) O::x_sqr(res, res);
        if (next >= 0) { typename O::T t = res; O::mul(t, t, f); res = t; }
        i = next - 1;
        if (next < 0) break;
    }
    O::conj(res);
    out = res;
}
// An ops struct may name a hook, O::before_exp_x(k), that runs before the chain's k-th ExpByX (k = 0..4): the lane-pair kernels' own struct
// lowers the wave's priority at one of them (pair_kernels.inc: PairYieldOps).  A struct without the member gets nothing.
template <class O, class = void> struct ExpXHook { static BLSMI_DEV void at(int) {} };
template <class O> struct ExpXHook<O, decltype(O::before_exp_x(0))> { static BLSMI_DEV void at(int k) { O::before_exp_x(k); } };
// pairing.go:79-129.  Computes r^(3(q^12-1)/r_order) in place; a non-invertible input (only 0)
// maps to 0 where the reference returns nil.
template <class O>
BLSMI_DEV void final_exp_chain(typename O::T& r) {
    typename O::T f2, y0, y1, y2, y3;
    O::inv(f2, r);
    O::conj(r);
    O::mul(r, r, f2);
    O::frob2(f2, r);
    O::mul(r, f2, r);
    const u64 x = BLSMI_X_ABS;
    O::cyc_sqr(y0, r);
    ExpXHook<O>::at(0); O::exp_x(y1, y0, x);
    ExpXHook<O>::at(1); O::exp_x(y2, y1, x >> 1);
    y3 = r; O::conj(y3);
    O::mul(y1, y1, y3);
    O::conj(y1);
    O::mul(y1, y1, y2);
    ExpXHook<O>::at(2); O::exp_x(y2, y1, x);
    ExpXHook<O>::at(3); O::exp_x(y3, y2, x);
    O::conj(y1);
    O::mul(y3, y3, y1);
    O::conj(y1);
    O::frob3(y1, y1);
    O::frob2(y2, y2);
    O::mul(y1, y1, y2);
    ExpXHook<O>::at(4); O::exp_x(y2, y3, x);
    O::mul(y2, y2, y0);
    O::mul(y2, y2, r);
    O::mul(y1, y1, y2);
    O::frob1(y3, y3);
    O::mul(r, y1, y3);
}

BLSMI_DEV Fp12W cyc_sqr_run(const Fp12W& g, int m) {
    CycCompressedW c = cyc_compress(g);
    for (int j = 0; j < m; j++) c = cyc_compressed_sqr(c);
    Fp2S num, den;
    cyc_z1_fraction(c, num, den);
    return cyc_decompress(c, fp2_mul(num, fp2_store(fp2_inv(den))));
}
BLSMI_NOINLINE void exp_by_x(Fp12W& out, const Fp12W& f, u64 e);
// one tuple per lane / per lane pair: the out-of-line routines above; inside exp_by_x the squarings are expanded in line
struct Fp12Ops {
    using T = Fp12W;
    static constexpr int MIN_RUN = 12;
    static BLSMI_DEV void inv(T& r, const T& a) { nf_fp12_inv(r, a); }
    static BLSMI_DEV void mul(T& r, const T& a, const T& b) { nf_fp12_mul(r, a, b); }
    static BLSMI_DEV void cyc_sqr(T& r, const T& a) { nf_fp12_cyc_sqr(r, a); }
    static BLSMI_DEV void x_sqr(T& r, const T& a) { r = fp12_cyclotomic_sqr(a); }
    static BLSMI_DEV void x_sqr_run(T& r, const T& a, int m) { r = cyc_sqr_run(a, m); }
    static BLSMI_DEV void frob1(T& r, const T& a) { nf_fp12_frob1(r, a); }
    static BLSMI_DEV void frob2(T& r, const T& a) { nf_fp12_frob2(r, a); }
    static BLSMI_DEV void frob3(T& r, const T& a) { nf_fp12_frob3(r, a); }
    static BLSMI_DEV void conj(T& a) { fp12_conj_inplace(a); }
    static BLSMI_DEV void exp_x(T& r, const T& a, u64 e) { exp_by_x(r, a, e); }
};
BLSMI_NOINLINE void exp_by_x(Fp12W& out, const Fp12W& f, u64 e) { exp_by_x_loop<Fp12Ops>(out, f, e); }
// a value of the storage type (what a kernel loads) through the chain: converted once on the way in, widened on the way out
BLSMI_DEV void final_exponentiation(Fp12S& r) {
    Fp12W w = fp12_work(r);
    final_exp_chain<Fp12Ops>(w);
    r = fp12_widen(w);
}

