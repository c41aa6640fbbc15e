// k_fq12_seg.hip -- the segmented Fq12 product of the pairing products (blsmi 0.10: blsmi_pairing_product_batch*), in the LANE-ROW layout
// (row_body.inc): sixteen adjacent lanes per chunk, 4 chunks per 64-lane workgroup, the product of a chunk's values by r12_mul (three
// product times each).  A few thousand chunks already put a wave on every SIMD; one chunk per lane (k_fq12_prod_level) would leave the
// chip idle at the sizes the entry points are for.  The host cuts every segment into chunks (verify_host.inc: segsum_plan); the same
// kernel serves pass 1 (values = the Miller loops' hand-off buffer, `skip` marks the pairs with a point at infinity), the fold passes and
// the final pass (one "chunk" per segment, an empty one gives 1).
#ifndef BLSMI_ROW_WAVES
#define BLSMI_ROW_WAVES 2
#endif
#ifndef BLSMI_PAIR_CORE_CALL
#define BLSMI_PAIR_CORE_INLINE
#endif
#include "pairing.cuh"
#include "device_io.cuh"
namespace blsmi {
namespace pairl {
#include "row_body.inc"
}  // namespace pairl
}  // namespace blsmi

#define KERNEL_ROW __global__ void __launch_bounds__(WG, BLSMI_ROW_WAVES)
namespace P2 = blsmi::pairl;
constexpr int RT = WG / 16;                                              // chunks per workgroup

// the buffers are the Miller-loop hand-off's (k_pairing_row.hip: row_store12 / row_load12)
BLSMI_DEV int row_fq_index(int pr, int par) { return 2 * (3 * (pr & 1) + (pr >> 1)) + par; }
BLSMI_DEV P2::R12 row_load12(const i32* buf, size_t n, size_t t, int pr, int par) {
    P2::R12 f;
    f.c = P2::fp2_tight(P2::wrap(soa_load(buf, n, t, row_fq_index(pr < 6 ? pr : 0, par))));
    return f;
}

// dst[c] = product of src[lo[c] .. lo[c] + cnt[c]) without the positions whose skip byte is set (skip null: none); nothing left: 1.
// dst: record c of an nch-record hand-off buffer, and / or out_m384: the reference's in-memory FQ12 (72 u64 per record) -- either may be null.
// The loop's trip count and the skip test are the same on the sixteen lanes of a row (DPP exchanges stay inside a row), not across a wave.
KERNEL_ROW k_fq12_seg_prod_row(const i32* src, size_t nsrc, const u8* skip, const u64* lo, const u32* cnt, i32* dst, u64* out_m384, size_t nch) {
    const int par = threadIdx.x & 1, pr = (threadIdx.x >> 1) & 7;
    const size_t c = (size_t)blockIdx.x * RT + (threadIdx.x >> 4);
    const size_t cc = c < nch ? c : nch - 1;
    const size_t a = lo[cc];
    const size_t e = a + cnt[cc] < nsrc ? a + cnt[cc] : nsrc;              // (the plan never reaches past the buffer; nor does a bad one)
    P2::R12 acc = P2::r12_one();
    bool first = true;
    for (size_t k = a; k < e; k++) {
        if (skip && skip[k]) continue;
        const P2::R12 v = row_load12(src, nsrc, k, pr, par);
        acc = first ? v : P2::r12_mul(acc, v);
        first = false;
    }
    if (c >= nch || pr >= 6) return;
    if (dst) soa_store(dst, nch, c, row_fq_index(pr, par), fp_relabel<FpS::L, FpS::V>(acc.c.c));
    if (out_m384) store_m384(out_m384 + 72 * c + 6 * row_fq_index(pr, par), acc.c.c);
}

// dst[t] = a[t] * b[t] for the n records of two hand-off buffers, a lane row per product (the block checks of blsmi 0.12: a block's product
// of tuple-side Miller values times its signature side's).  dst / out_m384 as above: the final exponentiation's input in either form.
KERNEL_ROW k_fq12_mul_pairs_row(const i32* a, const i32* b, i32* dst, u64* out_m384, size_t n) {
    const int par = threadIdx.x & 1, pr = (threadIdx.x >> 1) & 7;
    const size_t t = (size_t)blockIdx.x * RT + (threadIdx.x >> 4);
    const size_t tt = t < n ? t : n - 1;
    const P2::R12 acc = P2::r12_mul(row_load12(a, n, tt, pr, par), row_load12(b, n, tt, pr, par));
    if (t >= n || pr >= 6) return;
    if (dst) soa_store(dst, n, t, row_fq_index(pr, par), fp_relabel<FpS::L, FpS::V>(acc.c.c));
    if (out_m384) store_m384(out_m384 + 72 * t + 6 * row_fq_index(pr, par), acc.c.c);
}

// The pairs a product leaves out: skip[k] = the caller's flags (bit 0: P_k, bit 1: Q_k at infinity; null: none) or an all-zero record.  Such a
// pair's records are replaced by the generators' so that the Miller kernels, which take no point at infinity, run on valid points; its value
// is then left out by the product.  g1 / g2: the call's own copies.
__global__ void __launch_bounds__(WG) k_pprod_skip(u8* g1, u8* g2, const u8* in_flags, const u8* gen1, const u8* gen2, u8* skip, size_t n) {
    const size_t t = (size_t)blockIdx.x * WG + threadIdx.x;
    if (t >= n) return;
    u32* p = reinterpret_cast<u32*>(g1) + 24 * t;
    u32* q = reinterpret_cast<u32*>(g2) + 48 * t;
    u32 a = 0, b = 0;
    for (int i = 0; i < 24; i++) a |= p[i];
    for (int i = 0; i < 48; i++) b |= q[i];
    const u8 f = (u8)(((in_flags ? in_flags[t] : 0) & 3) | (a ? 0 : 1) | (b ? 0 : 2));
    skip[t] = f;
    if (!f) return;
    const u32* s1 = reinterpret_cast<const u32*>(gen1);
    const u32* s2 = reinterpret_cast<const u32*>(gen2);
    for (int i = 0; i < 24; i++) p[i] = s1[i];
    for (int i = 0; i < 48; i++) q[i] = s2[i];
}

// is_one[j] = (value j == FQ12One), values in the reference's in-memory form (72 u64 each): c0.c0.c0 = FQOne, every other Fq zero.
// Sixteen lanes per value, nine words each.
__global__ void __launch_bounds__(WG) k_fq12_is_one_m384(const u64* vals, u8* is_one, size_t n) {
    const int l = threadIdx.x & 15;
    const size_t t = (size_t)blockIdx.x * (WG / 16) + (threadIdx.x >> 4);
    const size_t tt = t < n ? t : n - 1;
    const u32* w = reinterpret_cast<const u32*>(vals) + 144 * tt;
    u32 d = 0;
    for (int i = 0; i < 9; i++) { const int j = 9 * l + i; d |= w[j] ^ (j < 12 ? C_ONE_M384_WORDS[j] : 0u); }
    int e = d == 0 ? 1 : 0;
    e &= __shfl_xor(e, 1); e &= __shfl_xor(e, 2); e &= __shfl_xor(e, 4); e &= __shfl_xor(e, 8);
    if (t < n && l == 0) is_one[t] = (u8)e;
}
