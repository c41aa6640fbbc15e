// route_table.cc -- a driver of bls_amd/csrc/route.h for tests/test_routing.py (host only).  Reads one question a line from stdin,
//   <question> <kind> <n> <others> [option=value ...]
// (options: Tuning members; unnamed ones keep the library defaults) and prints the answer on one line.  Questions: verify, pairing,
// miller, final_exp, aggregate (layout + Miller records), side, prepared (does a table serve: verify / pairing / aggregate), hash
// (the hash of a Verify: path + SWU layout), hash_agg (the uncleared hash of a large g2pubs aggregate), blocks (the workgroups n tuples
// take in the single, pair, quad and row layouts).  Two questions are about the
// option table itself (tests/test_options.py):
//   options                                       one line per row: member, blsmi_set_option name or -, variable or -, run-time / fixed, default
//   env [explicit=member,...] [VARIABLE=value ...]  every member after apply_env over that environment, the named rows set through the API
#include "../../bls_amd/csrc/route.h"
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

using namespace blsmi_route;

static const char* name(Layout l) { const char* s[] = {"wave", "row", "quad", "pair", "single"}; return s[(int)l]; }
static const char* name(Side x) { const char* s[] = {"none", "wave", "row"}; return s[(int)x]; }
static const char* name(HashPath p) { const char* s[] = {"lat", "g1_lane", "g1_quad", "g2_oct", "g2_row", "g2_quad", "g2_pair", "plain"}; return s[(int)p]; }
static const char* name(Swu w) { const char* s[] = {"waves", "rows", "lanes"}; return s[(int)w]; }

static void print_options() {
    const Tuning dflt;
    for (const Option& o : options)
        std::cout << o.member << " " << (o.set == Set::option ? o.member : "-") << " " << (o.env ? o.env : "-") << " " << (o.set == Set::fixed ? "fixed" : "run-time") << " "
                  << value_of(dflt, o) << "\n";
}
static bool print_env(std::istringstream& in) {
    std::map<std::string, std::string> vars;
    uint64_t mask = 0;
    std::string kv;
    while (in >> kv) {
        const size_t eq = kv.find('=');
        if (eq == std::string::npos) return false;
        if (kv.compare(0, eq, "explicit") != 0) { vars[kv.substr(0, eq)] = kv.substr(eq + 1); continue; }
        std::istringstream names(kv.substr(eq + 1));
        for (std::string m; std::getline(names, m, ',');) {
            int row = 0;
            while (row < n_options && m != options[row].member) row++;
            if (row == n_options) return false;
            mask |= (uint64_t)1 << row;
        }
    }
    Tuning t;
    apply_env(t, mask, [&](const char* name) { auto it = vars.find(name); return it == vars.end() ? (const char*)nullptr : it->second.c_str(); });
    for (const Option& o : options) std::cout << o.member << "=" << value_of(t, o) << " ";
    std::cout << "\n";
    return true;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string q, kv;
        int kind; size_t n, others;
        if (!(in >> q)) return 2;
        if (q == "options") { print_options(); continue; }
        if (q == "env") { if (!print_env(in)) { std::cerr << "bad line " << line << "\n"; return 2; } continue; }
        if (!(in >> kind >> n >> others)) return 2;
        Tuning t;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            if (eq == std::string::npos || set_by_name(t, kv.substr(0, eq).c_str(), std::atoll(kv.c_str() + eq + 1), false) < 0) { std::cerr << "bad option " << kv << "\n"; return 2; }
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
        else if (q == "blocks")
            std::cout << tuple_blocks(Layout::single, n) << " " << tuple_blocks(Layout::pair, n) << " " << tuple_blocks(Layout::quad, n) << " " << tuple_blocks(Layout::row, n);
        else { std::cerr << "bad question " << q << "\n"; return 2; }
        std::cout << "\n";
    }
    return 0;
}
