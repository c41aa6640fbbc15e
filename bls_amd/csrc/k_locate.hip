// k_locate.hip -- the housekeeping kernels of the block-locating randomised verification (blsmi 0.12: blsmi_g?pubs_*verify*_batch_rlc_locate,
// rlc_host.hpp) and of its grouped form (blsmi 0.13: ..._rlc_grouped_locate, whose blocks are the cells of cell_plan.h): the signature-side
// pairs of the block checks, the verdict byte of every block / cell, and the gathers / the scatter that move the tuples of the failing
// ones into dense buffers for the per-tuple stage and their verdicts back.  The product of a block's Miller values with its signature
// side's is k_fq12_mul_pairs_row (k_fq12_seg.hip).
// Also here: the weights of the randomised pairing-product batches (blsmi 0.17) and the route of their block-locating form (blsmi 0.18).
#include "tower.cuh"
#include "device_io.cuh"

// The B pairs whose Miller values stand for the signature side of the block equations: (-S_b, G2gen) for g2pubs (kind 0, S_b 96 bytes),
// (-G1gen, S_b) otherwise (S_b 192 bytes).  Where S_b is at infinity (s_inf[b], or the all-zero record) the pair is the generators' -- the
// Miller kernels take no point at infinity -- and bad[b] = 1: the block's equation is not trusted.
KERNEL2 k_locate_sig_pairs(int kind, const u8* sums, const u8* s_inf, const u8* gen1, const u8* gen2, u8* g1, u8* g2, u8* bad, size_t nb) {
    const size_t b = (size_t)blockIdx.x * WG + threadIdx.x;
    if (b >= nb) return;
    const u32 sw = kind == 0 ? 24 : 48;
    const u32* s = reinterpret_cast<const u32*>(sums) + (size_t)sw * b;
    u32 any = 0;
    for (u32 i = 0; i < sw; i++) any |= s[i];
    const bool inf = s_inf[b] != 0 || any == 0;
    bad[b] = inf ? 1 : 0;
    const u8* p = (kind == 0 && !inf) ? reinterpret_cast<const u8*>(s) : gen1;
    const u8* q = (kind != 0 && !inf) ? reinterpret_cast<const u8*>(s) : gen2;
    u32* o1 = reinterpret_cast<u32*>(g1) + (size_t)24 * b;
    u32* o2 = reinterpret_cast<u32*>(g2) + (size_t)48 * b;
    const u32* p32 = reinterpret_cast<const u32*>(p);
    const u32* q32 = reinterpret_cast<const u32*>(q);
    for (int i = 0; i < 12; i++) o1[i] = p32[i];
    store_be48(reinterpret_cast<u8*>(o1 + 12), fp_neg(load_be48(p + 48)));  // (a point of odd order has y != 0; store_be48 writes the canonical q - y)
    for (int i = 0; i < 48; i++) o2[i] = q32[i];
}

// fail[b] = 1 unless block b's equation held (is_one[b]), its sum was a point (bad[b] == 0) and none of its tuples is flagged in either of
// the two flag arrays (the inputs', the scaled points'); block b is the tuples [b * block, min(n, (b + 1) * block)).  Sixteen lanes per
// block: the flag bytes of a block are contiguous, lane l reads bytes l, l + 16, ...
KERNEL2 k_locate_block_fail(const u8* flags, const u8* flags2, size_t n, size_t block, const u8* bad, const u8* is_one, u8* fail, size_t nb) {
    const u32 l = threadIdx.x & 15;
    const size_t b = (size_t)blockIdx.x * (WG / 16) + (threadIdx.x >> 4);
    const size_t bb = b < nb ? b : nb - 1;
    const size_t lo = bb * block, hi = n - lo > block ? lo + block : n;
    u32 f = 0;
    for (size_t i = lo + l; i < hi; i += 16) f |= (u32)flags[i] | flags2[i];
    f |= __shfl_xor(f, 1); f |= __shfl_xor(f, 2); f |= __shfl_xor(f, 4); f |= __shfl_xor(f, 8);
    if (b < nb && l == 0) fail[b] = (f || bad[b] || !is_one[b]) ? 1 : 0;
}

// The same for the cells of a grouped call: cell c is the tuples perm[cell_off[c] .. cell_off[c + 1]) -- ragged, and scattered over the call's
// flag bytes, so every lane goes through perm (the uniform stride above does not serve).  cell_bad: the flag byte of the cell's key sum;
// flags2 may be null (this form scales no point per tuple).  Sixteen lanes per cell, lane l takes positions l, l + 16, ... of its cell; the
// OR across the sixteen stays inside their DPP row.  n: the tuples of the call, every perm entry below it.
KERNEL2 k_locate_cell_fail(const u8* flags, const u8* flags2, const u32* perm, const u64* cell_off, const u8* cell_bad, const u8* bad, const u8* is_one, u8* fail, size_t n, size_t nc) {
    const u32 l = threadIdx.x & 15;
    const size_t c = (size_t)blockIdx.x * (WG / 16) + (threadIdx.x >> 4);
    const size_t cc = c < nc ? c : nc - 1;
    const u64 lo = cell_off[cc], hi = cell_off[cc + 1];
    u32 f = 0;
    for (u64 k = lo + l; k < hi; k += 16) {
        const u32 i = perm[k];
        if (i >= n) { f = 1; continue; }                                   // (the host's plan never has one: such a cell would fail, nothing is read)
        f |= flags[i];
        if (flags2) f |= flags2[i];
    }
    f |= __shfl_xor(f, 1); f |= __shfl_xor(f, 2); f |= __shfl_xor(f, 4); f |= __shfl_xor(f, 8);
    if (c < nc && l == 0) fail[c] = (f || cell_bad[c] || bad[c] || !is_one[c]) ? 1 : 0;
}

// dst record r = src record idx[r] for records of q 16-byte pieces (96 bytes: 6, 192 bytes: 12), a lane per piece: the q lanes of a record
// are neighbours and read it whole.  The host has built the indices (locate_plan.h: locate_positions); buffers are 16-byte aligned.
KERNEL2 k_gather_records16(const uint4* src, const u32* idx, uint4* dst, u32 q, size_t n) {
    const size_t t = (size_t)blockIdx.x * WG + threadIdx.x;
    if (t >= (size_t)q * n) return;
    const size_t r = t / q;
    dst[t] = src[(size_t)idx[r] * q + (t - r * q)];
}
// dst[r] = src[idx[r]] (the caller's flag bytes of the gathered tuples) / dst[idx[r]] = src[r] (their verdicts back into the call's)
KERNEL2 k_gather_bytes(const u8* src, const u32* idx, u8* dst, size_t n) {
    const size_t r = (size_t)blockIdx.x * WG + threadIdx.x;
    if (r < n) dst[r] = src[idx[r]];
}
KERNEL2 k_scatter_bytes(const u8* src, const u32* idx, u8* dst, size_t n) {
    const size_t r = (size_t)blockIdx.x * WG + threadIdx.x;
    if (r < n) dst[idx[r]] = src[r];
}

// The weights and flags of a randomised pairing-product batch (blsmi 0.17: blsmi_pairing_product_batch_rlc*, rlc_host.hpp), a lane per pair:
// w[k] = r[item_of[k]], the scalar of the pair's item, addressed like the point as the weighted segmented sum wants it, and pflag[k] in the
// form blsmi_pairing_product_batch takes its flags -- bit 0: P_k is at infinity (the caller's flag or the all-zero record), bit 1: its table
// entry tab[group_of[k]] is the all-zero record.  The sums read bit 0 (any set bit leaves the pair out: a pair of a dropped group adds
// nothing either way), the per-item path gets the byte as it is.  tab: the call's compacted table (16-byte aligned); g1 may be a caller's
// buffer, read in 16-byte pieces where its address allows (the same for the whole grid).  The host has built item_of and group_of.
KERNEL2 k_pprod_rlc_weights(const u8* g1, const u8* in_flags, const uint4* tab, const u32* group_of, const u32* item_of, const u64* r, u64* w, u8* pflag, size_t np) {
    const size_t k = (size_t)blockIdx.x * WG + threadIdx.x;
    if (k >= np) return;
    u32 a = 0, b = 0;
    if ((reinterpret_cast<uintptr_t>(g1) & 15) == 0) {
        const uint4* p = reinterpret_cast<const uint4*>(g1) + 6 * k;
        for (int i = 0; i < 6; i++) { const uint4 v = p[i]; a |= v.x | v.y | v.z | v.w; }
    } else {
        const u32* p = reinterpret_cast<const u32*>(g1) + 24 * k;
        for (int i = 0; i < 24; i++) a |= p[i];
    }
    const uint4* q = tab + (size_t)12 * group_of[k];
    for (int i = 0; i < 12; i++) { const uint4 v = q[i]; b |= v.x | v.y | v.z | v.w; }
    pflag[k] = (u8)(((in_flags ? in_flags[k] : 0) & 1) | (a ? 0 : 1) | (b ? 0 : 2));
    w[k] = r[item_of[k]];
}

// The cells of a block-locating pairing-product batch into block order (blsmi 0.18: blsmi_pairing_product_batch_rlc_locate*, rlc_host.hpp;
// pprod_locate_plan.h has the slots), in one launch between the sums and the Miller loops: slot s gets the 96-byte sum of cell sum_of[s]
// and the 192-byte record of compacted table entry entry_at[s] in dense arrays, and the skip rule of k_pprod_skip is applied on the way --
// a sum at infinity (its flag byte, or the all-zero record: bit 0) or an all-zero entry (bit 1) leaves skip[s] != 0 and the generators in
// the slot, so that the Miller kernels run on valid points and the block's product leaves the value out.  Sixteen lanes per slot, 16-byte
// pieces: lanes 0..5 carry the sum, lanes 0..11 the entry, so the lanes of one record are neighbours and read it whole; the two ORs stay
// inside the sixteen.  The host has built the indices (every sum_of[s] < nc, every entry_at[s] < ne; one beyond would be skipped, nothing
// read); sums, tab, gen1, gen2, g1, g2 are 16-byte aligned.  No lane writes beyond slot nc - 1.
KERNEL2 k_pprod_cell_route(const uint4* sums, const u8* s_inf, const uint4* tab, const u32* sum_of, const u32* entry_at, const uint4* gen1, const uint4* gen2,
                           uint4* g1, uint4* g2, u8* skip, size_t nc, size_t ne) {
    const u32 l = threadIdx.x & 15;
    const size_t s = (size_t)blockIdx.x * (WG / 16) + (threadIdx.x >> 4);
    const size_t ss = s < nc ? s : nc - 1;
    const u32 c = sum_of[ss], e = entry_at[ss];
    const bool in = c < nc && e < ne;
    uint4 p = make_uint4(0, 0, 0, 0), q = make_uint4(0, 0, 0, 0);
    if (in && l < 6) p = sums[(size_t)6 * c + l];
    if (in && l < 12) q = tab[(size_t)12 * e + l];
    u32 a = p.x | p.y | p.z | p.w, b = q.x | q.y | q.z | q.w;
    a |= __shfl_xor(a, 1); a |= __shfl_xor(a, 2); a |= __shfl_xor(a, 4); a |= __shfl_xor(a, 8);
    b |= __shfl_xor(b, 1); b |= __shfl_xor(b, 2); b |= __shfl_xor(b, 4); b |= __shfl_xor(b, 8);
    const u8 f = (u8)(((!in || a == 0 || s_inf[c]) ? 1 : 0) | ((!in || b == 0) ? 2 : 0));
    if (s >= nc) return;
    if (f) { if (l < 6) p = gen1[l]; if (l < 12) q = gen2[l]; }
    if (l < 6) g1[(size_t)6 * s + l] = p;
    if (l < 12) g2[(size_t)12 * s + l] = q;
    if (l == 0) skip[s] = f;
}
