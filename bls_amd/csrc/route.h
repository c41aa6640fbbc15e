// route.h -- which kernels a call runs (host only, no HIP).  Every answer is a pure function of the call's size, the options it started
// with (Tuning, the snapshot CtxLease takes: blsmi.hip, tuning_now) and the tuples other calls had in flight on its device when it first
// asked (blsmi.hip: call_load).  A call asks each question once and hands the answer to every stage it concerns.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace blsmi_route {

// The options a kernel choice reads, as plain values; the defaults are the library's (its option atomics start from them, blsmi.hip,
// where the measurements behind them are noted).
struct Tuning {
    size_t lat_max = 8192, quad_max = 16384, quad_min = 5632, row_min = 2048, row_max = 8192;   // settable while running
    bool crowd_quad = true; size_t crowd_floor = 1536, assume_load = 0;
    size_t hash_row_min = 2048, hash_row_max = 4096, hash_quad_min = 4097, hash_quad_max = 16384;
    size_t hash_oct_min = 2048, hash_oct_max = 7168, hash_g1_quad_min = 1280, hash_g1_quad_max = 32768, swu_row_max = 4096;
    bool row_side = true, row_side_g2pubs = true;
    bool agg_cofactor_pow = true, msm_sort = true, lat_rolled = true, dup_force_sort = false, mul_subgroup = true;
    bool pair_layout = true, use_gen_lines = true, hash_g2_pair = true, hash_g1_split = true;   // fixed at initialisation (environment)
    size_t swu_wave_max = 512, fixed_wave_max = 2048;
    long long sig_side_max = -1;                                           // -1: the per-package defaults (sig_side)
    size_t rlc_min = 32768;                                                // randomised batch verification: below this many tuples, the per-tuple path
    size_t segsum_chunk = 0;                                               // segmented sums: positions per chunk and lane (0: from the total count, verify_host.inc: segsum_auto_chunk)
};

// One tuple per WAVE (k_lat.hip), per DPP ROW of sixteen lanes, per lane QUAD, per lane PAIR, or per lane (BLSMI_LAYOUT=single, and the
// one-lane kernels of what has no other layout)
enum class Layout : uint8_t { wave, row, quad, pair, single };
enum class Call : uint8_t { pairing, verify, aggregate };

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
