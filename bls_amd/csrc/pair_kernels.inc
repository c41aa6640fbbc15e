// pair_kernels.inc -- pairing kernels in the lane-pair layout (fp2_pair.inc): two adjacent lanes per tuple,
// 32 tuples per 64-lane workgroup, 256 registers per lane so that two waves share each SIMD.
#ifndef BLSMI_PAIR_WAVES
#define BLSMI_PAIR_WAVES 2
#endif
#define KERNEL_PAIR __global__ void __launch_bounds__(WG, BLSMI_PAIR_WAVES)
namespace P2 = blsmi::pairl;
struct PairG1 { FpS x, y; };
struct PairG2 { P2::Fp2S x, y; };
constexpr int PT = WG / 2;                                              // tuples per workgroup

// The yield.  A 65 536-tuple grid is exactly two waves on each of the 1 024 SIMDs, and VALU issue between the two goes by priority, then AGE
// (MI355X guide, "two waves per SIMD"): at equal priority the wave in slot 0 left at 0.59 of the kernel's span on every SIMD and the other ran
// the last 0.41 alone -- the second wave bought a few per cent (DESIGN 3p; tools/wave_census.py, profiles/r16_wave_yield.log).  So every wave of
// the kernels below enters at priority 1 and the leader goes down to 0 once most of its own work is done (fp.cuh: pair_yield_drop -- the wave
// in the odd slot, the one that lags, keeps its 1): the partner catches up, the leader's remaining work fills the slots the partner leaves,
// and both stay on the SIMD until nearly the end (first exit at 0.93 / 0.98 of the span, Miller loop / final exponentiation).
// Levels 1 and 0 only: the hash kernels' 2 (fp.cuh: hash_prio) keeps outranking a Miller kernel beside them.  s_setprio ignores EXEC: each drop
// sits in wave-uniform control flow (the bit walk's loop index, a kernel argument, a hardware register).  -DBLSMI_PAIR_YIELD=0: no s_setprio in
// these kernels (A/B).  Kernels with it: k_miller1_pair / k_miller1h_pair, k_miller2_pair, k_final_exp_pair, k_final_exp_is_one_pair.  Without:
// k_miller1x2_pair (half the waves), the prepared-table loops, the debug kernels.
#ifndef BLSMI_PAIR_YIELD
#define BLSMI_PAIR_YIELD 1
#endif
#ifndef BLSMI_PAIR_YIELD_MILLER
#define BLSMI_PAIR_YIELD_MILLER 50                                      // of the 62 bits x_bit_walk walks (a 63rd doubling follows them)
#endif
#ifndef BLSMI_PAIR_YIELD_FE
#define BLSMI_PAIR_YIELD_FE 4                                           // before the fifth of the chain's five ExpByX: 0.8 of the kernel's instructions
#endif
constexpr int PAIR_YIELD_MILLER_BITS = BLSMI_PAIR_YIELD ? BLSMI_PAIR_YIELD_MILLER : 0;
constexpr int PAIR_YIELD_FE_EXP_X = BLSMI_PAIR_YIELD_FE;
BLSMI_DEV void pair_yield_enter() {
#if BLSMI_PAIR_YIELD
    __builtin_amdgcn_s_setprio(1);
#endif
}
// the lane-pair layout's operations (pairing_body.inc: Fp12Ops) with the drop before one ExpByX of final_exp_chain
struct PairYieldOps : P2::Fp12Ops {
    static BLSMI_DEV void before_exp_x(int k) { if (k == PAIR_YIELD_FE_EXP_X) pair_yield_drop(); }
};
BLSMI_DEV void final_exponentiation_yield(P2::Fp12W& f) {                // on the chain's own type: the kernels below convert what they load once
#if BLSMI_PAIR_YIELD
    P2::final_exp_chain<PairYieldOps>(f);
#else
    P2::final_exp_chain<P2::Fp12Ops>(f);
#endif
}

// Diagnostic builds only (tools/build_variant.sh ... -DBLSMI_WAVE_CENSUS, read by tools/wave_census.py; never the product build): the
// kernels that yield leave one record per wave -- where it ran, when it entered, when it left -- in a __device__ array of this unit.
#ifdef BLSMI_WAVE_CENSUS
constexpr int CENSUS_WAVES = 4096, CENSUS_WORDS = 4;
#ifdef BLSMI_PAIR_FE_ONLY
#define BLSMI_CENSUS_BUF blsmi_census_fe
#define BLSMI_CENSUS_READ blsmi_census_read_fe
#else
#define BLSMI_CENSUS_BUF blsmi_census_miller
#define BLSMI_CENSUS_READ blsmi_census_read_miller
#endif
__device__ unsigned long long BLSMI_CENSUS_BUF[CENSUS_WAVES * CENSUS_WORDS];
extern "C" __attribute__((visibility("default"))) int BLSMI_CENSUS_READ(unsigned long long* out) {   // CENSUS_WAVES x CENSUS_WORDS words to the host
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(BLSMI_CENSUS_BUF), sizeof(BLSMI_CENSUS_BUF));
}
struct WaveCensus {
    u64 t0;
    BLSMI_DEV WaveCensus() : t0(__builtin_amdgcn_s_memrealtime()) {}
    BLSMI_DEV void leave(int kernel) const {
        const u64 t1 = __builtin_amdgcn_s_memrealtime();
        const u32 hw = __builtin_amdgcn_s_getreg(4 | (31 << 11)), xcc = __builtin_amdgcn_s_getreg(20 | (31 << 11));   // HW_ID, XCC_ID: all 32 bits
        if (threadIdx.x == 0 && blockIdx.x < CENSUS_WAVES) {                // one wave per workgroup
            unsigned long long* rec = BLSMI_CENSUS_BUF + (size_t)blockIdx.x * CENSUS_WORDS;
            rec[0] = (u64)hw | ((u64)xcc << 32); rec[1] = t0; rec[2] = t1; rec[3] = (u64)kernel + 1;
        }
    }
};
#else
struct WaveCensus { BLSMI_DEV void leave(int) const {} };
#endif

template <int WORDS>
BLSMI_DEV void tile_load_pair(u32* lds, const u8* gbase, size_t first, size_t n) {
    const u32* g = reinterpret_cast<const u32*>(gbase) + first * WORDS;
    const size_t valid = (n - first < (size_t)PT ? n - first : (size_t)PT) * WORDS;
    for (int idx = threadIdx.x; idx < PT * WORDS; idx += WG)
        if ((size_t)idx < valid) lds[(idx / WORDS) * (WORDS + 1) + (idx % WORDS)] = g[idx];
    __syncthreads();
}
template <int WORDS>
BLSMI_DEV void tile_store_pair(const u32* lds, u8* gbase, size_t first, size_t n) {
    __syncthreads();
    u32* g = reinterpret_cast<u32*>(gbase) + first * WORDS;
    const size_t valid = (n - first < (size_t)PT ? n - first : (size_t)PT) * WORDS;
    for (int idx = threadIdx.x; idx < PT * WORDS; idx += WG)
        if ((size_t)idx < valid) g[idx] = lds[(idx / WORDS) * (WORDS + 1) + (idx % WORDS)];
}
BLSMI_DEV void pair_store12(i32* buf, size_t n, size_t t, int par, const P2::Fp12S& f) {
    const FpS* c = reinterpret_cast<const FpS*>(&f);                     // 6 Fp per lane: coefficient `par` of the 6 Fq2
#pragma unroll
    for (int j = 0; j < 6; j++) soa_store(buf, n, t, 2 * j + par, c[j]);
}
BLSMI_DEV P2::Fp12S pair_load12(const i32* buf, size_t n, size_t t, int par) {
    P2::Fp12S f;
    FpS* c = reinterpret_cast<FpS*>(&f);
#pragma unroll
    for (int j = 0; j < 6; j++) c[j] = soa_load(buf, n, t, 2 * j + par);
    return f;
}
#ifndef BLSMI_PAIR_FE_ONLY
template <bool EXACT> BLSMI_DEV void miller1_pair_body(const u8* g1, const u8* g2, i32* fbuf, size_t n) {
    __shared__ u32 lds[PT * 49];
    const int par = threadIdx.x & 1, loc = threadIdx.x >> 1;
    const size_t first = (size_t)blockIdx.x * PT;
    const size_t t = first + loc;
    const int rec = (t < n) ? loc : (int)(n - 1 - first);
    PairG1 p[1]; PairG2 q[1];
    const WaveCensus census;
    pair_yield_enter();
    tile_load_pair<24>(lds, g1, first, n);
    p[0].x = lds_be48(lds + rec * 25); p[0].y = lds_be48(lds + rec * 25 + 12);
    __syncthreads();
    tile_load_pair<48>(lds, g2, first, n);
    q[0].x = P2::wrap(lds_be48(lds + rec * 49 + 12 * par));
    q[0].y = P2::wrap(lds_be48(lds + rec * 49 + 24 + 12 * par));
    P2::Fp12S f;
    if constexpr (EXACT) P2::miller_loop<1, false, EXACT, false, PAIR_YIELD_MILLER_BITS>(f, p, q);
    else {
        __shared__ i32 lds_r[45 * WG];                                     // the running point (pairing_body.inc: lds_put_proj)
        __syncthreads();                                                   // the input tile above shares nothing with it, but keep the waves of a larger group in step
        P2::miller_loop<1, false, EXACT, false, PAIR_YIELD_MILLER_BITS>(f, p, q, nullptr, nullptr, lds_r);
    }
    if (t < n) pair_store12(fbuf, n, t, par, f);
    census.leave(0);
}
// k_miller1_pair: the reference's Miller value (MillerLoop, pairing.go:16-75); k_miller1h_pair: a Miller value with the same
// final exponentiation, by the cheaper homogeneous steps (Pairing, VerifyAggregate)
KERNEL_PAIR k_miller1_pair(const u8* g1, const u8* g2, i32* fbuf, size_t n) { miller1_pair_body<true>(g1, g2, fbuf, n); }
KERNEL_PAIR k_miller1h_pair(const u8* g1, const u8* g2, i32* fbuf, size_t n) { miller1_pair_body<false>(g1, g2, fbuf, n); }
#endif
#ifndef BLSMI_PAIR_MILLER_ONLY
KERNEL_PAIR k_final_exp_pair(const i32* fbuf, u64* out, size_t n, int mode) {
    __shared__ u32 lds[PT * 145];
    const int par = threadIdx.x & 1, loc = threadIdx.x >> 1;
    const size_t first = (size_t)blockIdx.x * PT;
    const size_t t = first + loc;
    const size_t tt = t < n ? t : n - 1;
    const WaveCensus census;
    pair_yield_enter();
    P2::Fp12W f = P2::fp12_work(pair_load12(fbuf, n, tt, par));
    if (mode == 0) final_exponentiation_yield(f);
    const FpW* c = reinterpret_cast<const FpW*>(&f);
    for (int j = 0; j < 6; j++) {
        u32 w[12];
        fp_to_mont384_words(c[j], w);
#pragma unroll
        for (int k = 0; k < 12; k++) lds[loc * 145 + 12 * (2 * j + par) + k] = w[k];
    }
    tile_store_pair<144>(lds, reinterpret_cast<u8*>(out), first, n);
    census.leave(1);
}
#endif
#ifndef BLSMI_PAIR_FE_ONLY

// The Miller loops of a VerifyAggregate: the product of n pairings is wanted, so a lane pair takes TWO consecutive tuples and
// runs them as one 2-pair loop (shared squarings, the step's two lines multiplied together first): m = ceil(n / 2) values,
// 72 % of the instructions of n one-pair loops.  The last lane pair of an odd n runs a one-pair loop.
KERNEL_PAIR k_miller1x2_pair(const u8* g1, const u8* g2, i32* fbuf, size_t n, size_t m) {
    const int par = threadIdx.x & 1;
    const size_t t = (size_t)blockIdx.x * PT + (threadIdx.x >> 1);
    const size_t tt = t < m ? t : m - 1;
    const size_t i0 = 2 * tt, i1 = 2 * tt + 1 < n ? 2 * tt + 1 : i0;
    PairG1 p[2]; PairG2 q[2];
    p[0].x = load_be48(g1 + 96 * i0); p[0].y = load_be48(g1 + 96 * i0 + 48);
    p[1].x = load_be48(g1 + 96 * i1); p[1].y = load_be48(g1 + 96 * i1 + 48);
    q[0].x = P2::wrap(load_be48(g2 + 192 * i0 + 48 * par)); q[0].y = P2::wrap(load_be48(g2 + 192 * i0 + 96 + 48 * par));
    q[1].x = P2::wrap(load_be48(g2 + 192 * i1 + 48 * par)); q[1].y = P2::wrap(load_be48(g2 + 192 * i1 + 96 + 48 * par));
    P2::Fp12S f;
    __shared__ i32 lds_r[45 * WG];                                         // one running point per lane pair (pairing_body.inc: lds_put_proj)
    if (__all(2 * tt + 1 < n)) P2::miller_loop<2, false, false>(f, p, q, nullptr, nullptr, lds_r);
    else {                                                                 // the wave that holds the odd tuple out
        P2::Fp12S f2, f1;
        P2::miller_loop<2, false, false>(f2, p, q, nullptr, nullptr, lds_r);
        PairG1 p1[1] = {p[0]}; PairG2 q1[1] = {q[0]};
        P2::miller_loop<1, false, false>(f1, p1, q1, nullptr, nullptr, lds_r);
        const i32 both = 2 * tt + 1 < n ? -1 : 0;
        FpS* a = reinterpret_cast<FpS*>(&f2); const FpS* b = reinterpret_cast<const FpS*>(&f1);
        for (int j = 0; j < 6; j++) a[j] = fp_select(both, a[j], b[j]);
        f = f2;
    }
    if (t < m) pair_store12(fbuf, m, t, par, f);
}

// CompareTwoPairings in the pair layout (see k_miller2): strides in bytes, 0 = broadcast record
KERNEL_PAIR k_miller2_pair(const u8* p0, size_t sp0, const u8* q0, size_t sq0, const u8* p1, size_t sp1, const u8* q1, size_t sq1, i32* fbuf, size_t n, const i32* pre) {
    __shared__ u32 lds[PT * 49];
    const int par = threadIdx.x & 1, loc = threadIdx.x >> 1;
    const size_t first = (size_t)blockIdx.x * PT;
    const size_t t = first + loc;
    const int rec = (t < n) ? loc : (int)(n - 1 - first);
    PairG1 p[2]; PairG2 q[2];
    const WaveCensus census;
    pair_yield_enter();
    if (sp0) { tile_load_pair<24>(lds, p0, first, n); p[0].x = lds_be48(lds + rec * 25); p[0].y = lds_be48(lds + rec * 25 + 12); __syncthreads(); }
    else { p[0].x = load_be48(p0); p[0].y = load_be48(p0 + 48); }
    if (sq0) { tile_load_pair<48>(lds, q0, first, n); q[0].x = P2::wrap(lds_be48(lds + rec * 49 + 12 * par)); q[0].y = P2::wrap(lds_be48(lds + rec * 49 + 24 + 12 * par)); __syncthreads(); }
    else { q[0].x = P2::wrap(load_be48(q0 + 48 * par)); q[0].y = P2::wrap(load_be48(q0 + 96 + 48 * par)); }
    tile_load_pair<24>(lds, p1, first, n);
    p[1].x = lds_be48(lds + rec * 25); p[1].y = fp_store(fp_neg(lds_be48(lds + rec * 25 + 12)));   // -P1
    __syncthreads();
    tile_load_pair<48>(lds, q1, first, n);
    q[1].x = P2::wrap(lds_be48(lds + rec * 49 + 12 * par)); q[1].y = P2::wrap(lds_be48(lds + rec * 49 + 24 + 12 * par));
    (void)sp1; (void)sq1;
    P2::Fp12S f;
    __shared__ i32 lds_r[45 * WG];                                         // pair 1's running point (pairing_body.inc: lds_put_proj)
    __syncthreads();
    if (pre) P2::miller_loop<2, true, false, false, PAIR_YIELD_MILLER_BITS>(f, p, q, pre, nullptr, lds_r);   // only the verdict leaves: homogeneous steps
    else P2::miller_loop<2, false, false, false, PAIR_YIELD_MILLER_BITS>(f, p, q, nullptr, nullptr, lds_r);
    if (t < n) pair_store12(fbuf, n, t, par, f);
    census.leave(2);
}
#endif
#ifndef BLSMI_PAIR_MILLER_ONLY
KERNEL_PAIR k_final_exp_is_one_pair(const i32* fbuf, const u8* inf_flags, u8* ok, size_t n) {
    const int par = threadIdx.x & 1, loc = threadIdx.x >> 1;
    const size_t t = (size_t)blockIdx.x * PT + loc;
    const size_t tt = t < n ? t : n - 1;
    const WaveCensus census;
    pair_yield_enter();
    P2::Fp12W f = P2::fp12_work(pair_load12(fbuf, n, tt, par));
    final_exponentiation_yield(f);
    const bool one = P2::fp12_eq(f, P2::fp12_one());
    if (t < n && par == 0) ok[t] = (one && !(inf_flags && inf_flags[t])) ? 1 : 0;
    census.leave(3);
}
#endif
