// locate_plan.h -- the host plan of the block-locating randomised verification (blsmi 0.12: blsmi_g?pubs_*verify*_batch_rlc_locate; host
// only, no HIP, so that tests/native/locate_plan.cc runs it natively).  The n tuples of a call are cut into contiguous blocks of `block`
// tuples, the last one possibly shorter.  The tuple side leaves one Miller value per tuple, or one per two consecutive tuples in the quad
// and pair layouts (route.h: aggregate_route); `block` is even so that a block border is a record border there too.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace blsmi_route {

// block == 0 in a call: the next even number >= max(64, ceil(n / 256)).  Up to 16 384 tuples blocks of 64, beyond at most 256 blocks
// (the sweep at 65 536 tuples is flat from 64 to 1 024, so the rule stands as first written).
inline size_t locate_auto_block(size_t n) {
    const size_t b = std::max<size_t>(64, n / 256 + (n % 256 != 0));
    return b + (b & 1);
}
// what a caller may pass as `block`
inline bool locate_block_valid(size_t block) { return block == 0 || (block >= 2 && (block & 1) == 0); }

struct LocatePlan {
    size_t n = 0, block = 0;
    std::vector<uint64_t> tup_off;   // B + 1 borders in tuples, from 0 to n, strictly increasing
    std::vector<uint64_t> rec_off;   // B + 1 borders in Miller values: the same, or with `halved` ceil(border / 2)
    size_t blocks() const { return tup_off.size() - 1; }
};
// block: even and >= 2 (the caller has resolved 0); halved: two consecutive tuples leave one value.  n == 0 gives no block.
inline void locate_plan(size_t n, size_t block, bool halved, LocatePlan& p) {
    p.n = n; p.block = block;
    p.tup_off.assign(1, 0); p.rec_off.assign(1, 0);
    for (size_t lo = 0; lo < n;) {
        const size_t hi = n - lo > block ? lo + block : n;
        p.tup_off.push_back(hi);
        p.rec_off.push_back(halved ? hi / 2 + (hi & 1) : hi);
        lo = hi;
    }
}
// The tuple positions of the blocks whose byte in `fail` is not zero, ascending: what the per-tuple stage gathers, verifies and scatters.
inline void locate_positions(const LocatePlan& p, const uint8_t* fail, std::vector<uint32_t>& pos) {
    pos.clear();
    for (size_t b = 0; b < p.blocks(); b++)
        if (fail[b]) for (uint64_t i = p.tup_off[b]; i < p.tup_off[b + 1]; i++) pos.push_back((uint32_t)i);
}

}  // namespace blsmi_route
