// route.h -- which kernels a call runs (host only, no HIP).  Every answer is a pure function of the call's size, the options it started
// with (Tuning, the snapshot CtxLease takes: blsmi.hip, tuning_now) and the tuples other calls had in flight on its device when it first
// asked (blsmi.hip: call_load).  A call asks each question once and hands the answer to every stage it concerns.
// An option is DEFINED here and nowhere else: its default is its member initialiser in Tuning; how it is set -- by blsmi_set_option, by its
// environment variable and the rule that is read by, after initialisation or not -- is its row of `options` below (the store: blsmi.hip, g_opt).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>

namespace blsmi_route {

// The options a kernel choice reads, as plain values with the library's defaults and the measurements behind them.
struct Tuning {
    // Layouts by batch size, pairings and verifies alike (tools/midsize.py): one tuple per WAVE up to min(lat_max, quad_min) tuples, one per lane
    // QUAD up to quad_max (16 384 tuples = one wave on every SIMD), one per lane PAIR beyond (65 536 fill the chip twice over).
    size_t lat_max = 8192;     // the wave and the pair path meet at ~10 000 tuples (tools/crossover.py: 8192 pairings 8.4 ms against 10.7, 16 384: 16.4 against 11.3); read by every call, written rarely
    size_t quad_max = 16384;   // 0: no quad kernels
    size_t quad_min = 5632;    // the quad kernels take over from the latency path here already (pairings: 5.9 ms flat against 1 ms per 1 024 tuples; verifies 8.7 against 1.5)
    // A fourth layout between the wave and the quad (k_pairing_row.hip): one tuple per DPP ROW of sixteen lanes.  row_min .. row_max tuples of a LONE
    // caller take it: 4 096 tuples are one wave on every SIMD there (a quarter of the SIMDs in the quad layout, four waves of 3.3 x the instructions
    // on the one-tuple-per-wave path).  A Pairing call's row range reaches half again as far (pairing_layout): with no hash beside its two kernels the
    // row kernels stay ahead of the quad kernels' flat 5.7 ms up to 12 288 tuples (three waves per SIMD: 5.34 ms; verifies cross at ~10 000: 12 288
    // g2pubs verifies 8.96 against 7.95 ms).  max 0: off.
    size_t row_min = 2048;     // (tools/midsize4.py: 2 048 pairings 2.08 against 2.21 ms on the wave path, g1pubs verifies 4.45 against 4.72, g2pubs 3.66 against 3.57; 1 024: 2.05 against 1.54)
    size_t row_max = 8192;     // (8 192 pairings 4.0 ms against the quad kernels' flat 5.7; 12 288: 6+ against 5.7)
    // The thresholds above are a LONE caller's: one tuple per wave finishes 4 096 pairings in 4.3 ms where the quad kernels take their flat 6 ms.
    // Callers that arrive together are a different matter (tools/midsize_concurrency.py): the latency path saturates the chip at 1.04 M pairings/s
    // whatever the number of calls in flight (its waves are bounded by LDS, 9 per CU), the quad kernels at 2.8 M/s (two 8 192-tuple calls take
    // the 6 ms of one).  So the choice goes by what the DEVICE carries: a call of at least crowd_floor tuples takes the quad kernels when its
    // tuples plus those of the other calls in flight pass the lone crossover (floor 1 536: four callers x 2 048 pairings 7.9 -> 6.1 ms a call; at 1 024
    // the sum never passes the crossover with four contexts); the row layout is a lone call's (the quad kernels spend fewer lane-instructions per
    // tuple: 12.6 M against 18 M).  A call registers its tuples at its first layout question and keeps the answer's input for its whole life (one
    // call never sees two different loads); ~CtxLease takes them off again.
    bool crowd_quad = true; size_t crowd_floor = 1536;
    size_t assume_load = 0;    // test hook: tuples pretended to be in flight from other calls
    size_t hash_row_min = 2048, hash_row_max = 4096;          // HashG2 of this many messages clears its cofactor in the lane-row layout (k_clear_h2_row; max 0: never)
    size_t hash_quad_min = 4097, hash_quad_max = 16384;       // ... four lanes per message (k_clear_h2_quad)
    size_t hash_oct_min = 2048, hash_oct_max = 7168;          // ... eight lanes per message (k_clear_h2_oct, oct_g2.inc); takes precedence over the row and quad tails
    size_t hash_g1_quad_min = 1280, hash_g1_quad_max = 32768; // HashG1's tail four lanes per message (k_hash_g1_finish_quad)
    size_t swu_row_max = 4096; // the SWU maps of HashG1 / HashG2 run a ROW of sixteen lanes per map (k_swu_g?_rows) above swu_wave_max and up to here; 0: never
    bool row_side = true;      // a Verify in the row layout runs its signature side beside the hash (verify_host.inc)
    bool row_side_g2pubs = true;   // ... for g2pubs too (the signature side over the generator's table as a kernel of its own: 4 096 tuples 3.23 against 3.55 ms, verify_host.inc)
    bool agg_cofactor_pow = true, msm_sort = true;   // large g2pubs aggregates raise their Miller product to 1 - x instead of clearing n hash points; device radix sort against the exact histogram passes
    bool lat_rolled = true;    // 0: small Pairing calls take the STRAIGHT-LINE copy of their level program (pairing1s) instead of the one with rolled squaring runs (A/B)
    bool dup_force_sort = false;   // test hook: the duplicate screen's fallback on every call
    bool mul_subgroup = true;  // scalar multiplication through the endomorphisms (multiplicands in the subgroup); 0: plain ladder
    size_t combine_mid_max = 8192; // concurrent Verify calls of BLSMI_COMBINE_MAX <= n < this many tuples merge into one launch (verify_host.inc); 0: never
    size_t rlc_min = 32768;    // randomised batch verification: below this many tuples, the per-tuple path
    size_t segsum_chunk = 0;   // segmented sums: positions per chunk and lane (0: from the total count, verify_host.inc: segsum_auto_chunk)
    bool pair_layout = true, use_gen_lines = true;   // 0: one tuple per lane instead of two lanes per tuple (BLSMI_LAYOUT=single); 0: the generator's lines are recomputed per tuple (A/B switch)
    bool hash_g1_split = true, hash_g2_pair = true, cofac2_pair = true;   // 0: the one-lane HashG1 / HashG2 kernel, the fused one-lane HashG2WithDomain kernel
    size_t hash_g2_pair_redo_every = 0;   // tests: exercise the redo pass of the lane-pair HashG2
    size_t swu_wave_max = 512; // the smallest hashes / decompressions run one WAVE per field exponentiation up to here (measured: 0.68 against 0.96 ms at 512 messages, 1.18 against 0.98 at 1 024)
    size_t fixed_wave_max = 2048;  // PrivToPub over the generators' fixed-base tables: a wave per multiplication up to here
    long long sig_side_max = -1;   // -1: the per-package defaults (sig_side)
    size_t side_max = 131072, msm_bucket_min = (size_t)1 << 17;   // Deserialize + Verify: the decompressions and the hash on three streams up to here (verify_host.inc); an MSM of at least this many points takes the bucket method
};

// How a row's environment variable is read when it is set (unset: the default); apply_env spells each rule out.  They differ for historical
// reasons and are part of the interface as they are.
enum class Env : uint8_t { none, number, integer, off_at_0, atoi, present, is_0, not_0, not_single };
// How a row changes after initialisation: not at all, through blsmi_set_option under its member's name, or through a blsmi_set_* function of its own
enum class Set : uint8_t { fixed, option, setter };
struct Option {
    const char* member;
    size_t Tuning::*num; bool Tuning::*flag; long long Tuning::*integer;   // exactly one is not null
    Set set; const char* env; Env rule;
    constexpr Option(const char* m, size_t Tuning::*p, Set s, const char* e = nullptr, Env r = Env::none) : member(m), num(p), flag(nullptr), integer(nullptr), set(s), env(e), rule(r) {}
    constexpr Option(const char* m, bool Tuning::*p, Set s, const char* e = nullptr, Env r = Env::none) : member(m), num(nullptr), flag(p), integer(nullptr), set(s), env(e), rule(r) {}
    constexpr Option(const char* m, long long Tuning::*p, Set s, const char* e = nullptr, Env r = Env::none) : member(m), num(nullptr), flag(nullptr), integer(p), set(s), env(e), rule(r) {}
};
#define BLSMI_OPT(m, ...) Option(#m, &Tuning::m, __VA_ARGS__)
constexpr Option options[] = {
    BLSMI_OPT(lat_max, Set::setter, "BLSMI_LAT_MAX", Env::number),             // blsmi_set_latency_threshold
    BLSMI_OPT(quad_max, Set::setter, "BLSMI_QUAD_MAX", Env::number),           // blsmi_set_quad_threshold
    BLSMI_OPT(quad_min, Set::fixed, "BLSMI_QUAD_MIN", Env::number),
    BLSMI_OPT(row_min, Set::setter, "BLSMI_ROW_MIN", Env::number), BLSMI_OPT(row_max, Set::setter, "BLSMI_ROW_MAX", Env::number),   // blsmi_set_row_threshold
    BLSMI_OPT(crowd_quad, Set::option, "BLSMI_CROWD_QUAD", Env::off_at_0),
    BLSMI_OPT(crowd_floor, Set::option, "BLSMI_CROWD_FLOOR", Env::number),
    BLSMI_OPT(assume_load, Set::option),
    BLSMI_OPT(hash_row_min, Set::option), BLSMI_OPT(hash_row_max, Set::option),
    BLSMI_OPT(hash_quad_min, Set::option), BLSMI_OPT(hash_quad_max, Set::option),
    BLSMI_OPT(hash_oct_min, Set::option), BLSMI_OPT(hash_oct_max, Set::option),
    BLSMI_OPT(hash_g1_quad_min, Set::option), BLSMI_OPT(hash_g1_quad_max, Set::option),
    BLSMI_OPT(swu_row_max, Set::option),
    BLSMI_OPT(row_side, Set::option, "BLSMI_ROW_SIDE", Env::off_at_0),
    BLSMI_OPT(row_side_g2pubs, Set::option),
    BLSMI_OPT(agg_cofactor_pow, Set::option, "BLSMI_AGG_COFACTOR_POW", Env::off_at_0),
    BLSMI_OPT(msm_sort, Set::option, "BLSMI_MSM_SORT", Env::off_at_0),
    BLSMI_OPT(lat_rolled, Set::option, "BLSMI_LAT_ROLLED", Env::off_at_0),
    BLSMI_OPT(dup_force_sort, Set::option, "BLSMI_DUP_FORCE_SORT", Env::present),
    BLSMI_OPT(mul_subgroup, Set::setter, "BLSMI_MUL_GENERIC", Env::is_0),      // blsmi_set_mul_assume_subgroup; the variable is the inverse
    BLSMI_OPT(combine_mid_max, Set::option, "BLSMI_COMBINE_MID_MAX", Env::number),
    BLSMI_OPT(rlc_min, Set::option, "BLSMI_RLC_MIN", Env::number),
    BLSMI_OPT(segsum_chunk, Set::option, "BLSMI_SEGSUM_CHUNK", Env::number),
    BLSMI_OPT(pair_layout, Set::fixed, "BLSMI_LAYOUT", Env::not_single),
    BLSMI_OPT(use_gen_lines, Set::fixed, "BLSMI_GEN_LINES", Env::not_0),
    BLSMI_OPT(hash_g2_pair, Set::fixed, "BLSMI_HASH_G2_PAIR", Env::atoi), BLSMI_OPT(hash_g1_split, Set::fixed, "BLSMI_HASH_G1_SPLIT", Env::atoi),
    BLSMI_OPT(hash_g2_pair_redo_every, Set::fixed, "BLSMI_HASH_G2_PAIR_REDO_EVERY", Env::number),
    BLSMI_OPT(cofac2_pair, Set::fixed, "BLSMI_COFAC2_PAIR", Env::atoi),
    BLSMI_OPT(swu_wave_max, Set::fixed, "BLSMI_SWU_WAVE_MAX", Env::number), BLSMI_OPT(fixed_wave_max, Set::fixed, "BLSMI_FIXED_WAVE_MAX", Env::number),
    BLSMI_OPT(sig_side_max, Set::fixed, "BLSMI_SIG_SIDE_MAX", Env::integer),
    BLSMI_OPT(side_max, Set::fixed, "BLSMI_SIDE_MAX", Env::number), BLSMI_OPT(msm_bucket_min, Set::fixed, "BLSMI_MSM_BUCKET_MIN", Env::number),
};
#undef BLSMI_OPT
constexpr int n_options = (int)(sizeof options / sizeof options[0]);
static_assert(n_options <= 64, "one bit per row in a uint64_t mask");

inline long long value_of(const Tuning& t, const Option& o) { return o.num ? (long long)(t.*o.num) : o.flag ? (long long)(t.*o.flag) : t.*o.integer; }
// the row of a member (the blsmi_set_* functions of Set::setter rows), -1: none
inline int row_of(size_t Tuning::*m) { for (int i = 0; i < n_options; i++) if (options[i].num && options[i].num == m) return i; return -1; }
inline int row_of(bool Tuning::*m) { for (int i = 0; i < n_options; i++) if (options[i].flag && options[i].flag == m) return i; return -1; }
// Set the row whose member is called `name` -- with runtime_only, only a row blsmi_set_option may set -- and return it; -1: no such row.
// Sizes take max(0, value), switches value != 0.
inline int set_by_name(Tuning& t, const char* name, long long value, bool runtime_only) {
    for (int i = 0; i < n_options; i++) {
        const Option& o = options[i];
        if (strcmp(o.member, name) != 0) continue;
        if (runtime_only && o.set != Set::option) return -1;
        if (o.num) t.*o.num = (size_t)std::max(0LL, value); else if (o.flag) t.*o.flag = value != 0; else t.*o.integer = value;
        return i;
    }
    return -1;
}
// The environment, through env(variable) -> value or null: every row with a variable whose bit in explicit_mask is clear gets the variable's
// value by the row's rule, or its default where the variable is unset.  Rows set through the API (their bit is set) keep what they hold.
template <class Getenv>
inline void apply_env(Tuning& t, uint64_t explicit_mask, Getenv&& env) {
    const Tuning dflt;
    for (int i = 0; i < n_options; i++) {
        const Option& o = options[i];
        if (o.rule == Env::none || (explicit_mask >> i & 1)) continue;
        const char* v = env(o.env);
        if (!v) { if (o.num) t.*o.num = dflt.*o.num; else if (o.flag) t.*o.flag = dflt.*o.flag; else t.*o.integer = dflt.*o.integer; continue; }
        switch (o.rule) {
            case Env::none: break;
            case Env::number: t.*o.num = (size_t)strtoull(v, nullptr, 10); break;
            case Env::integer: t.*o.integer = atoll(v); break;                       // may be negative
            case Env::off_at_0: t.*o.flag = v[0] != '0'; break;                      // off iff the FIRST character is '0'
            case Env::atoi: t.*o.flag = atoi(v) != 0; break;                         // "yes" is off
            case Env::present: t.*o.flag = true; break;                              // on whatever the value, "0" included
            case Env::is_0: t.*o.flag = strcmp(v, "0") == 0; break;                  // the whole value
            case Env::not_0: t.*o.flag = strcmp(v, "0") != 0; break;
            case Env::not_single: t.*o.flag = strcmp(v, "single") != 0; break;
        }
    }
}

// One tuple per WAVE (k_lat.hip), per DPP ROW of sixteen lanes, per lane QUAD, per lane PAIR, or per lane (BLSMI_LAYOUT=single, and the
// one-lane kernels of what has no other layout)
enum class Layout : uint8_t { wave, row, quad, pair, single };
enum class Call : uint8_t { pairing, verify, aggregate };
// Tuples a workgroup of 64 lanes serves in a lane layout, and the workgroups n tuples take (a wave-layout call launches a wave per tuple)
constexpr size_t tuples_per_block(Layout l) { return l == Layout::single ? 64 : l == Layout::pair ? 32 : l == Layout::quad ? 16 : l == Layout::row ? 4 : 1; }
constexpr unsigned tuple_blocks(Layout l, size_t n) { return (unsigned)((n + tuples_per_block(l) - 1) / tuples_per_block(l)); }

// The hand-overs are a lone caller's; a call of at least crowd_floor tuples also counts the `others` in flight on its device.
inline bool crowded(size_t n, const Tuning& t) { return t.crowd_quad && n >= t.crowd_floor; }
inline size_t lone_max(const Tuning& t) { return std::min(t.lat_max, t.quad_min); }
inline bool row_fits(size_t n, size_t hi, const Tuning& t, size_t others) {
    if (!crowded(n, t)) others = 0;
    if (!t.pair_layout || hi == 0 || n > hi || n < t.row_min) return false;
    return !(others > 0 && n + others > lone_max(t));
}
// Verify: row across the row range (lone calls), quad up to quad_max once past the lone crossover, wave up to lat_max, pair beyond
inline Layout verify_layout(size_t n, const Tuning& t, size_t others) {
    if (row_fits(n, t.row_max, t, others)) return Layout::row;
    if (t.pair_layout && n <= t.quad_max && n + (crowded(n, t) ? others : 0) > lone_max(t)) return Layout::quad;
    if (n <= t.lat_max) return Layout::wave;
    return t.pair_layout ? Layout::pair : Layout::single;
}
// Pairing (mode 0): as Verify, its row range half again as far (no hash beside its kernels); MillerLoop (mode 1): wave up to lat_max
inline Layout pairing_layout(int mode, size_t n, const Tuning& t, size_t others) {
    if (mode == 1) return n <= t.lat_max ? Layout::wave : t.pair_layout ? Layout::pair : Layout::single;
    const Layout v = verify_layout(n, t, others);
    return v != Layout::wave && row_fits(n, t.row_max + t.row_max / 2, t, others) ? Layout::row : v;
}
inline Layout final_exp_layout(size_t n, const Tuning& t, size_t others) {
    return row_fits(n, t.row_max, t, others) ? Layout::row : n <= t.lat_max ? Layout::wave : Layout::single;
}
// VerifyAggregate's Miller loops: up to lat_max a row or a wave per tuple; beyond, two tuples per lane quad up to 2 quad_max, per lane pair above
inline Layout aggregate_layout(size_t n, const Tuning& t, size_t others) {
    if (n <= t.lat_max) return row_fits(n, t.row_max, t, others) ? Layout::row : Layout::wave;
    if (!t.pair_layout) return Layout::single;
    return (n + 1) / 2 <= t.quad_max ? Layout::quad : Layout::pair;
}
// Prepared keys' tables serve the lane-pair kernels only; every other layout gathers the keys' affine records.  Verify and
// VerifyAggregate also read the generator's prepared lines there (BLSMI_GEN_LINES=0: they gather).
inline bool prepared_tables_serve(Call c, Layout l, const Tuning& t) { return l == Layout::pair && (c == Call::pairing || t.use_gen_lines); }

// A Verify's signature side (verify_host.inc: verify_sig_side_start): a wave per tuple for the smallest calls, a row per tuple across the
// row range.  Never where prepared tables serve: that is the pair layout.
enum class Side : uint8_t { none, wave, row };
inline Side sig_side(int kind, size_t n, Layout l, const Tuning& t) {
    if (n == 0) return Side::none;
    if (l == Layout::row) return t.row_side && (kind != 0 || t.row_side_g2pubs) ? Side::row : Side::none;
    const size_t lim = t.sig_side_max >= 0 ? (size_t)t.sig_side_max : (kind == 0 ? (size_t)48 : (size_t)320);
    return l == Layout::wave && n <= lim ? Side::wave : Side::none;
}

// A hash of n messages (kind 0: HashG1, 1: HashG2, 2: HashG2WithDomain).  lat: the maps, then a level program one message per wave;
// g1_lane / g1_quad: HashG1's two maps on two lanes, its tail a lane / four lanes per message; g2_oct / g2_row / g2_quad: HashG2's maps and
// isogeny a lane pair per message, the cofactor clearing eight / sixteen / four lanes per message; g2_pair: a lane pair throughout; plain:
// the one-lane kernels.  swu: the maps of the lat and g1 paths a wave, a row of sixteen lanes, or two lanes per map.
enum class HashPath : uint8_t { lat, g1_lane, g1_quad, g2_oct, g2_row, g2_quad, g2_pair, plain };
enum class Swu : uint8_t { waves, rows, lanes };
struct HashRoute { HashPath path; Swu swu; };
// l: the Verify layout of n tuples; g1_clear == false: HashG1 without its cofactor clearing (large g2pubs aggregates); beside_side: the
// signature side's row kernel runs beside the hash, whose maps then stay two lanes each (few waves, the chip left to the side kernel)
inline HashRoute hash_route(int kind, size_t n, Layout l, bool g1_clear, bool beside_side, const Tuning& t) {
    auto in = [n](size_t lo, size_t hi) { return n >= lo && n <= hi; };
    const bool g2 = kind == 1 && t.hash_g2_pair, g2_tail = g2 && t.pair_layout;
    const bool oct = g2_tail && in(t.hash_oct_min, t.hash_oct_max);
    const bool row = g2_tail && !oct && in(t.hash_row_min, t.hash_row_max);
    const bool quad = g2_tail && !oct && !row && in(t.hash_quad_min, t.hash_quad_max);
    const bool g1_split = kind == 0 && t.hash_g1_split && n <= 2 * t.quad_max;
    const bool g1_quad = g1_split && g1_clear && in(t.hash_g1_quad_min, t.hash_g1_quad_max);
    // the row layout hashes on the level programs while they beat the mid-size kernels' flat times; the quad layout never does
    const size_t lat_max = oct || row || quad || g1_quad ? 0 : l == Layout::row ? (kind == 0 ? (size_t)3584 : (size_t)3072) : t.lat_max / 2;
    if (n <= lat_max && n <= t.lat_max / 2 && g1_clear && l != Layout::quad) {
        const bool waves = n <= (kind == 2 ? t.swu_wave_max / 4 : t.swu_wave_max);
        return {HashPath::lat, waves ? Swu::waves : !beside_side && kind != 2 && n <= t.swu_row_max ? Swu::rows : Swu::lanes};
    }
    if (g1_split) return {g1_quad ? HashPath::g1_quad : HashPath::g1_lane, !beside_side && n > t.swu_wave_max && n <= t.swu_row_max ? Swu::rows : Swu::lanes};
    if (g2) return {oct ? HashPath::g2_oct : row ? HashPath::g2_row : quad ? HashPath::g2_quad : HashPath::g2_pair, Swu::lanes};
    return {HashPath::plain, Swu::lanes};
}

// A Verify decides its layout, whether prepared tables serve it, its signature side (split_side == false: none, the signatures are not
// there yet) and its hash; a VerifyAggregate shard its Miller layout, the Miller values that leaves (two tuples share a loop in the quad
// and pair layouts), the tables and its hash.
struct VerifyRoute { Layout layout; bool tables; Side side; HashRoute hash; };
inline VerifyRoute verify_route(int kind, size_t n, bool prepared, bool split_side, const Tuning& t, size_t others) {
    const Layout l = verify_layout(n, t, others);
    const Side side = split_side ? sig_side(kind, n, l, t) : Side::none;
    return {l, prepared && kind == 0 && prepared_tables_serve(Call::verify, l, t), side, hash_route(kind, n, l, true, kind == 0 && side == Side::row, t)};
}
struct AggregateRoute { Layout layout; size_t records; bool tables; HashRoute hash; };
inline AggregateRoute aggregate_route(int kind, size_t n, bool prepared, bool g1_clear, const Tuning& t, size_t others) {
    const Layout l = aggregate_layout(n, t, others);
    return {l, l == Layout::quad || l == Layout::pair ? (n + 1) / 2 : n, prepared && kind == 0 && prepared_tables_serve(Call::aggregate, l, t),
            hash_route(kind, n, verify_layout(n, t, others), g1_clear, false, t)};
}

}  // namespace blsmi_route
