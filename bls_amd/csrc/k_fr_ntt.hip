// k_fr_ntt.hip -- interpolation over a coset in Fr on the device (blsmi 0.22): from the n = 2^l values of a polynomial over h <w> the n
// coefficients of its interpolant (blsmi_fr_coset_interp_batch*, and through it blsmi_kzg_verify_cell_batch*, rlc_host.hpp).  The arithmetic
// is fr.h, the transform's indices and butterfly are fr_ntt.h, which run natively as well.
//     a = the inverse DFT of the values, 1 / n included;        c_i = h^(-i) a_i
// One launch behind k_fr_inv over the shifts.  A workgroup of 256 lanes holds a tile of 512 elements in LDS, word-major as the tree of
// k_fr_eval.hip (word k of slot s at k * 512 + s: a lane's eight words lie in eight rows, consecutive lanes in consecutive banks), 16 KB:
//   n <= 512   512 / n whole items per tile (n = 1: 256 items, a lane each, and no stage); l stages of 256 butterflies, a lane each
//   n = 1024   one item in two tiles one after the other -- in bit-reversed position order the first nine stages stay within either half --
//              whose results wait in registers; the last stage pairs position k with k + 512, both in the same lane
// Bit-reversed input (order 1) goes into LDS where it lies, natural input (order 0) is permuted on the way in; the output is natural.
// No atomics, plain stores; a third small LDS array gathers the items' non-canonical flags.
#include <hip/hip_runtime.h>
#include "fr_ntt.h"
#include "fr_dev_io.cuh"                                                       // scalars and table elements in device memory

#define NTT_WG 256
#define NTT_TILE 512

namespace {
__device__ inline Fr tile_get(const u32* lds, u32 slot) {
    Fr o;
#pragma unroll
    for (int k = 0; k < 8; k++) o.w[k] = lds[k * NTT_TILE + slot];
    return o;
}
__device__ inline void tile_put(u32* lds, u32 slot, const Fr& v) {
#pragma unroll
    for (int k = 0; k < 8; k++) lds[k * NTT_TILE + slot] = v.w[k];
}
// One tile of a group through its tl stages in LDS: loads its values (one product per value brings it into Montgomery form with the 1 / n
// applied), runs the stages -- lane l butterfly l of the tile, its twiddle by the butterfly's index within the item as one of the whole
// transform of size 2^log2n -- and hands the lane the elements of its slots l and l + 256.  n = 1 has no stage and one slot per lane.
struct NttShape { u32 log2n, tl, per; int order; bool al; size_t m; };
__device__ inline void tile_pass(u32* lds, u32* s_nc, const NttShape& sh, u32 T, const u8* vals, const u32* tab, const Fr& factor, size_t item0, Fr& r0, Fr& r1) {
    const u32 l = threadIdx.x, tl = sh.tl;
    const size_t n = (size_t)1 << sh.log2n;
    for (u32 q = 0; q < sh.per; q++) {
        const u32 u = l + NTT_WG * q, pos = u & ((1u << tl) - 1), it = u >> tl;
        if (item0 + it >= sh.m) continue;
        const u32 src = sh.log2n > 9 ? (sh.order ? T * NTT_TILE + u : 2 * u + T) : pos;   // the value's position within its item
        const u32 slot = sh.order ? u : (u - pos) + blsmi_fr::ntt_bitrev(pos, tl);        // natural input is permuted on the way in
        u32 v[8];
        load_scalar(vals + 32 * ((item0 + it) * n + src), sh.al, v);
        if (!blsmi_fr::is_canonical(v)) s_nc[it] = 1;                          // (every writer writes the same value)
        tile_put(lds, slot, blsmi_fr::ntt_load_scaled(v, factor));
    }
    __syncthreads();
    for (u32 s = 0; s < tl; s++) {
        const u32 lo = blsmi_fr::ntt_lower(l, s), hi = blsmi_fr::ntt_partner(lo, s);
        if (item0 + (lo >> tl) < sh.m) {
            Fr a = tile_get(lds, lo), b = tile_get(lds, hi);
            blsmi_fr::ntt_butterfly(a, b, load_table(tab, blsmi_fr::ntt_twiddle(l & ((1u << tl >> 1) - 1), s, sh.log2n)));
            tile_put(lds, lo, a); tile_put(lds, hi, b);
        }
        __syncthreads();
    }
    r0 = tile_get(lds, l);
    if (sh.per == 2) r1 = tile_get(lds, l + NTT_WG);
    __syncthreads();                                                           // (the next tile, or the next group, overwrites the slots)
}
__device__ inline Fr pick(u32 e, const Fr& a, const Fr& b, const Fr& c, const Fr& d) {
    Fr o;
#pragma unroll
    for (int k = 0; k < 8; k++) o.w[k] = e == 0 ? a.w[k] : e == 1 ? b.w[k] : e == 2 ? c.w[k] : d.w[k];
    return o;
}
}  // namespace

// vals: m items of n = 2^log2n values, 32 big-endian bytes each, ANY 256-bit value taken mod r, read as 16-byte pieces when the buffer is
// 16-byte aligned, else byte by byte (the same for the whole grid); order 0: position i of an item is the value at h w^i, order 1: at
// h w^bitrev(i).  shifts: the m values h_j, hinv: their inverses as k_fr_inv left them (0 for 0), 4-byte aligned.  tab: the order-0 domain
// table of size n and n^-1 behind it (fr.h: domain_table).  coeffs[j][i]: the coefficient of X^i, fully reduced; shift_pow[j] (may be null):
// h_j^n mod r; flags[j] (may be null): bit 0: a value or the shift of item j was >= r, bit 1: h_j = 0 mod r.  Group g of items (and
// g + gridDim.x, ...) is the tile's 512 / n items, lane l its slots l and l + 256.  A workgroup reads all of its items before it writes any.
__global__ void __launch_bounds__(NTT_WG) k_fr_coset_interp(const u8* vals, const u8* shifts, const u8* hinv, const u32* tab, u32 log2n, int order, u8* coeffs, u8* shift_pow, u8* flags, size_t m) {
    __shared__ u32 lds[8 * NTT_TILE];
    __shared__ u32 s_nc[NTT_WG];
    const u32 l = threadIdx.x;
    const u32 n = (u32)1 << log2n;
    const u32 tl = log2n < 9 ? log2n : 9;                                      // stages in LDS; an item's positions within a tile: 2^tl
    const u32 ntile = log2n > 9 ? 2 : 1;                                       // tiles per group
    const u32 per = log2n == 0 ? 1 : 2;                                        // slots per lane and tile
    const u32 gitems = log2n > 9 ? 1 : (per * NTT_WG) >> log2n;                // items per group
    const size_t ngroups = (m + gitems - 1) / gitems;
    const bool al = (reinterpret_cast<uintptr_t>(vals) & 15) == 0;
    const Fr factor = blsmi_fr::ntt_scale_factor(load_table(tab, n));
    const NttShape sh{log2n, tl, per, order, al, m};
    for (size_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const size_t item0 = g * gitems;
        s_nc[l] = 0;
        __syncthreads();
        Fr a0 = blsmi_fr::zero(), a1 = a0, b0 = a0, b1 = a0;                   // the lane's elements: tile 0, tile 1
        tile_pass(lds, s_nc, sh, 0, vals, tab, factor, item0, a0, a1);
        if (ntile == 2) {                                                      // the last stage: positions k = l, l + 256 and k + 512
            tile_pass(lds, s_nc, sh, 1, vals, tab, factor, item0, b0, b1);
            blsmi_fr::ntt_butterfly(a0, b0, load_table(tab, (n - l) & (n - 1)));
            blsmi_fr::ntt_butterfly(a1, b1, load_table(tab, n - l - NTT_WG));
        }
        // scale by h^-i and store; the lane of an item's position 0 writes h^n and the flags
        for (u32 e = 0; e < per * ntile; e++) {
            const u32 u = l + NTT_WG * (e & 1), it = u >> tl;
            const u32 pos = (u & ((1u << tl) - 1)) + (e >> 1) * NTT_TILE;      // natural order: the coefficient's index
            const size_t j = item0 + it;
            if (j >= m) continue;
            u32 v[8];
            load_scalar4(hinv + 32 * j, v);
            const Fr c = blsmi_fr::mul(pick(e, a0, a1, b0, b1), blsmi_fr::ntt_pow_small(blsmi_fr::from_words(v), pos, log2n));
            blsmi_fr::to_words(c, v);
            store_scalar4(coeffs + 32 * (j * n + pos), v);
            if (pos == 0 && (shift_pow || flags)) {
                load_scalar4(shifts + 32 * j, v);
                const bool nc = !blsmi_fr::is_canonical(v);
                const Fr h = blsmi_fr::from_words(v);
                if (flags) flags[j] = (u8)(((nc || s_nc[it]) ? 1 : 0) | (blsmi_fr::is_zero(h) ? 2 : 0));
                if (shift_pow) {
                    blsmi_fr::to_words(blsmi_fr::ntt_pow_pow2(h, log2n), v);
                    store_scalar4(shift_pow + 32 * j, v);
                }
            }
        }
        __syncthreads();                                                       // (s_nc is cleared for the next group)
    }
}
