// route_table.cc -- a driver of bls_amd/csrc/route.h for tests/test_routing.py (host only).  Reads one question a line from stdin,
//   <question> <kind> <n> <others> [option=value ...]
// (options: Tuning members; unnamed ones keep the library defaults) and prints the answer on one line.  Questions: verify, pairing,
// miller, final_exp, aggregate (layout + Miller records), side, prepared (does a table serve: verify / pairing / aggregate), hash
// (the hash of a Verify: path + SWU layout), hash_agg (the uncleared hash of a large g2pubs aggregate).
#include "../../bls_amd/csrc/route.h"
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

using namespace blsmi_route;

static const char* name(Layout l) { const char* s[] = {"wave", "row", "quad", "pair", "single"}; return s[(int)l]; }
static const char* name(Side x) { const char* s[] = {"none", "wave", "row"}; return s[(int)x]; }
static const char* name(HashPath p) { const char* s[] = {"lat", "g1_lane", "g1_quad", "g2_oct", "g2_row", "g2_quad", "g2_pair", "plain"}; return s[(int)p]; }
static const char* name(Swu w) { const char* s[] = {"waves", "rows", "lanes"}; return s[(int)w]; }

static bool set(Tuning& t, const std::string& k, long long v) {
#define F(m) if (k == #m) { t.m = (decltype(t.m))v; return true; }
    F(lat_max) F(quad_max) F(quad_min) F(row_min) F(row_max) F(crowd_quad) F(crowd_floor) F(assume_load)
    F(hash_row_min) F(hash_row_max) F(hash_quad_min) F(hash_quad_max) F(hash_oct_min) F(hash_oct_max) F(hash_g1_quad_min) F(hash_g1_quad_max)
    F(swu_row_max) F(row_side) F(row_side_g2pubs) F(pair_layout) F(use_gen_lines) F(hash_g2_pair) F(hash_g1_split) F(swu_wave_max) F(sig_side_max)
#undef F
    return false;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string q, kv;
        int kind; size_t n, others;
        if (!(in >> q >> kind >> n >> others)) return 2;
        Tuning t;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            if (eq == std::string::npos || !set(t, kv.substr(0, eq), std::atoll(kv.c_str() + eq + 1))) { std::cerr << "bad option " << kv << "\n"; return 2; }
        }
        // the load a call sees: what other calls carry plus the "assume_load" test hook (blsmi.hip: call_load)
        const size_t load = others + t.assume_load;
        if (q == "verify") std::cout << name(verify_layout(n, t, load));
        else if (q == "pairing") std::cout << name(pairing_layout(0, n, t, load));
        else if (q == "miller") std::cout << name(pairing_layout(1, n, t, load));
        else if (q == "final_exp") std::cout << name(final_exp_layout(n, t, load));
        else if (q == "aggregate") { const AggregateRoute r = aggregate_route(kind, n, false, true, t, load); std::cout << name(r.layout) << " " << r.records; }
        else if (q == "side") std::cout << name(verify_route(kind, n, true, true, t, load).side);
        else if (q == "prepared")
            std::cout << verify_route(0, n, true, true, t, load).tables << " " << prepared_tables_serve(Call::pairing, pairing_layout(0, n, t, load), t) << " "
                      << aggregate_route(0, n, true, true, t, load).tables;
        else if (q == "hash") { const HashRoute h = verify_route(kind, n, false, true, t, load).hash; std::cout << name(h.path) << " " << name(h.swu); }
        else if (q == "hash_agg") { const HashRoute h = aggregate_route(kind, n, false, false, t, load).hash; std::cout << name(h.path) << " " << name(h.swu); }
        else { std::cerr << "bad question " << q << "\n"; return 2; }
        std::cout << "\n";
    }
    return 0;
}
