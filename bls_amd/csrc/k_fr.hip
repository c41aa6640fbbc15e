// k_fr.hip -- arithmetic mod r on the device (blsmi 0.19): the weighted segmented fold of scalars, blsmi_fr_wsum_segmented_u64*, and the
// housekeeping kernels of blsmi_groth16_verify_batch* (rlc_host.hpp), which folds its public inputs with it.  The arithmetic itself --
// the wide accumulator, its carry-resolving addition, the reduction mod r -- is fr_fold.h, which runs natively as well.
#include "tower.cuh"
#include "device_io.cuh"
#include "fr_fold.h"

#define FR_WG 256

// Pass 1 of the fold.  vals: rows of ncol scalars, 32 bytes big-endian each; w: one 64-bit weight per row; chunk ch is the rows
// [ch_lo[ch], ch_lo[ch] + ch_cnt[ch]) of ONE segment (the host's plan: fr_wsum_plan).  The outputs have cols = ncol + 1 columns, column 0 the
// weights' own sum -- a column whose value is one and is never loaded -- and column 1 + i the weighted sum of vals[.][i].  A workgroup takes
// one chunk and one tile of cw = min(cols, 256) columns: lane l is column l % cw of the tile, row l / cw of every R = 256 / cw rows, so the
// lanes of a row are neighbours and a workgroup reads R whole rows, contiguous, per step (two 16-byte loads per scalar; a caller's buffer
// that is not 16-byte aligned is read byte by byte, the same for the whole grid).  Every lane adds unreduced 64 x 256-bit products into
// twelve words; the R lanes of a column then meet in LDS, halving, every addition with its carries resolved; the chunk's unreduced
// twelve words per column go to part[(ch * cols + col) * 12 ..].  No atomics, nothing reduced mod r here.
__global__ void __launch_bounds__(FR_WG) k_fr_wsum_u64(const u8* vals, size_t ncol, const u64* w, const u64* ch_lo, const u32* ch_cnt, u32* part, size_t nch) {
    __shared__ u32 lds[blsmi_fr::ACC_WORDS * FR_WG];                          // word-major: word k of lane l at k * 256 + l
    const size_t cols = ncol + 1;
    const u32 cw = cols < FR_WG ? (u32)cols : FR_WG, R = FR_WG / cw;
    const size_t ntile = (cols + cw - 1) / cw;
    const size_t ch = blockIdx.x / ntile, tile = blockIdx.x - ch * ntile;
    const u32 l = threadIdx.x, ro = l / cw, cl = l - ro * cw;
    const size_t col = tile * cw + cl;
    const bool active = ch < nch && ro < R && col < cols;
    blsmi_fr::Acc acc; blsmi_fr::acc_zero(acc);
    if (active) {
        const u64 lo = ch_lo[ch]; const u32 cnt = ch_cnt[ch];
        const bool al = (reinterpret_cast<uintptr_t>(vals) & 15) == 0;
        for (u32 j = ro; j < cnt; j += R) {
            const u64 row = lo + j;
            u32 v[8] = {1, 0, 0, 0, 0, 0, 0, 0};
            if (col) {
                const u8* p = vals + ((size_t)row * ncol + (col - 1)) * 32;
                if (al) {
                    const uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1];
                    v[0] = __builtin_bswap32(b.w); v[1] = __builtin_bswap32(b.z); v[2] = __builtin_bswap32(b.y); v[3] = __builtin_bswap32(b.x);
                    v[4] = __builtin_bswap32(a.w); v[5] = __builtin_bswap32(a.z); v[6] = __builtin_bswap32(a.y); v[7] = __builtin_bswap32(a.x);
                } else blsmi_fr::load_be32(p, v);
            }
            blsmi_fr::acc_mul_add(acc, v, w[row]);
        }
    }
#pragma unroll
    for (int k = 0; k < blsmi_fr::ACC_WORDS; k++) lds[k * FR_WG + l] = acc.w[k];
    __syncthreads();
    u32 h = 1;
    while (h < R) h <<= 1;
    u32 live = R;                                                          // rows still holding a partial: ro < live
    for (h >>= 1; h >= 1; h >>= 1) {
        if (ro < h && ro + h < live) {                                     // (reads slots >= h, writes its own < h: no lane reads what another writes)
            blsmi_fr::Acc o;
#pragma unroll
            for (int k = 0; k < blsmi_fr::ACC_WORDS; k++) o.w[k] = lds[k * FR_WG + l + h * cw];
            blsmi_fr::acc_add(acc, o);
#pragma unroll
            for (int k = 0; k < blsmi_fr::ACC_WORDS; k++) lds[k * FR_WG + l] = acc.w[k];
        }
        __syncthreads();
        if (live > h) live = h;
    }
    if (active && ro == 0) {
        u32* o = part + (ch * cols + col) * blsmi_fr::ACC_WORDS;
#pragma unroll
        for (int k = 0; k < blsmi_fr::ACC_WORDS; k++) o[k] = acc.w[k];
    }
}

// Pass 2, a lane per output: output o = (segment s, column c) adds the partials of the segment's chunks seg_ch[s] .. seg_ch[s + 1] (none:
// zero), reduces the sum mod r -- the one reduction an output gets -- and writes it as 32 big-endian bytes at out + 32 o.
__global__ void __launch_bounds__(FR_WG) k_fr_wsum_fold(const u32* part, const u64* seg_ch, size_t cols, u8* out, size_t nout) {
    const size_t o = (size_t)blockIdx.x * FR_WG + threadIdx.x;
    if (o >= nout) return;
    const size_t s = o / cols, c = o - s * cols;
    blsmi_fr::Acc acc; blsmi_fr::acc_zero(acc);
    for (u64 ch = seg_ch[s]; ch < seg_ch[s + 1]; ch++) {
        blsmi_fr::Acc p;
        const u32* q = part + (ch * cols + c) * blsmi_fr::ACC_WORDS;
#pragma unroll
        for (int k = 0; k < blsmi_fr::ACC_WORDS; k++) p.w[k] = q[k];
        blsmi_fr::acc_add(acc, p);
    }
    u32 v[8];
    blsmi_fr::acc_reduce(acc, v);
    u32* d = reinterpret_cast<u32*>(out + 32 * o);                           // (out is the call's own or a caller's buffer: 4-byte aligned)
#pragma unroll
    for (int k = 0; k < 8; k++) d[k] = __builtin_bswap32(v[7 - k]);
}

// dst record i = minus the G2 record src[idx[i]] (affine, 192 bytes), a lane per record; the all-zero record stays all-zero.  The verifying
// key's beta, gamma, delta of blsmi_groth16_verify_batch*: e(P, -Q) = e(-P, Q), and three negations replace one per proof.
KERNEL2 k_g2_neg_records(const u8* src, const u32* idx, u8* dst, size_t n) {
    const size_t i = (size_t)blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    G2Aff a = load_g2(src + (size_t)192 * idx[i]);
    a.y.c0 = fp_neg(a.y.c0); a.y.c1 = fp_neg(a.y.c1);
    store_g2(dst + (size_t)192 * i, a);
}

// The four pairs of every item a Groth16 batch rechecks, dense, for blsmi_pairing_product_batch's own path: item t (dense) is proof
// items[t] = j, and its pairs are (A_j, B_j), (alpha, -beta), (L_t, -gamma), (C_j, -delta) -- proofs: A_j, C_j interleaved; L: the dense
// public-input points with their infinity bytes; tab: B_0 .. B_{m-1}, then -delta, -beta, -gamma.  Sixteen lanes per pair, 16-byte pieces
// (lanes 0..5 the G1 record, 0..11 the G2 record), the flag byte of the pair -- bit 0: the G1 point is infinite, bit 1: the G2 record is
// all-zero -- from the records themselves.  Every buffer is 16-byte aligned; no lane writes beyond pair 4 nre - 1.
KERNEL2 k_groth16_recheck_pairs(const uint4* proofs, const uint4* alpha, const uint4* L, const u8* L_inf, const uint4* tab, const u32* items, size_t m,
                                uint4* g1, uint4* g2, u8* flags, size_t nre) {
    const u32 l = threadIdx.x & 15;
    const size_t p = (size_t)blockIdx.x * (WG / 16) + (threadIdx.x >> 4);
    const size_t pp = p < 4 * nre ? p : 4 * nre - 1;
    const size_t t = pp >> 2; const u32 q = (u32)(pp & 3);
    const size_t j = items[t];
    const uint4* a = q == 0 ? proofs + 12 * j : q == 1 ? alpha : q == 2 ? L + 6 * t : proofs + 12 * j + 6;
    const uint4* b = tab + 12 * (q == 0 ? j : q == 1 ? m + 1 : q == 2 ? m + 2 : m);
    uint4 x = make_uint4(0, 0, 0, 0), y = make_uint4(0, 0, 0, 0);
    if (j < m && l < 6) x = a[l];
    if (j < m && l < 12) y = b[l];
    u32 ax = x.x | x.y | x.z | x.w, ay = y.x | y.y | y.z | y.w;
    ax |= __shfl_xor(ax, 1); ax |= __shfl_xor(ax, 2); ax |= __shfl_xor(ax, 4); ax |= __shfl_xor(ax, 8);
    ay |= __shfl_xor(ay, 1); ay |= __shfl_xor(ay, 2); ay |= __shfl_xor(ay, 4); ay |= __shfl_xor(ay, 8);
    if (p >= 4 * nre) return;
    if (l < 6) g1[6 * p + l] = x;
    if (l < 12) g2[12 * p + l] = y;
    if (l == 0) flags[p] = (u8)(((ax == 0 || (q == 2 && L_inf[t])) ? 1 : 0) | (ay == 0 ? 2 : 0));
}
