// k_kzg.hip -- the lift of a KZG batch (blsmi 0.20): out_j = A_j + [k_j] B_j, blsmi_g1_mul_add_batch[_dev], and the housekeeping kernels of
// blsmi_kzg_verify_batch* (rlc_host.hpp), which lifts W_j = C_j + [z_j] pi_j with it.
#include "tower.cuh"
#include "device_io.cuh"
#include "glv.cuh"

// One lane per item: the endomorphism ladder of k_g1_mul_glv on B_j (glv.cuh: B_j in the prime-order subgroup), ONE mixed addition of A_j
// into the Jacobian result -- A_j may be any curve point: the addition's special cases cover A_j infinite, [k] B infinite, A_j = [k] B (the
// doubling) and A_j = -[k] B (infinity) -- and the one inversion the ladder's kernel already pays.  a, b: affine records a_stride / b_stride
// bytes apart (0: one common record), 4-byte aligned; out: records out_stride bytes apart, so that a caller interleaves them with others.
// k_j is ANY 256-bit value: the decomposition k = k1 + k2 z^2 is an identity of integers (glv_model.py: k2 < 2^129 for every k below 2^256)
// and [z^2] B = -phi(B) for B of order r, hence [k] B = [k mod r] B with no reduction here.  An infinite result is the all-zero record and
// out_inf = 1.  The lanes behind n in the last wave repeat item n - 1 and write nothing.
__global__ void __launch_bounds__(WG, BLSMI_GLV_WAVES) k_g1_mul_add_glv(const u8* a, size_t a_stride, const u8* b, size_t b_stride, const u8* scalars,
                                                                        u8* out, size_t out_stride, u8* out_inf, size_t n) {
    const size_t t = (size_t)blockIdx.x * WG + threadIdx.x;
    const size_t tt = t < n ? t : n - 1;
    const G1Aff pb = load_g1(b + b_stride * tt);
    G1Jac acc = glv_mul<FpS>(pb, scalars + 32 * tt);
    const G1Aff pa = load_g1(a + a_stride * tt);                           // (read after the ladder: 25 words that need not live through it)
    acc = jac_add_affine_i(acc, pa);
    const G1Aff r = jac_to_affine(acc);
    if (t < n) { store_g1(out + out_stride * t, r); out_inf[t] = r.inf ? 1 : 0; }
}

// n copies of minus the G1 record at src (the all-zero record stays all-zero), a lane per copy: the multiplicand -G of the blocks' s_b and of
// the rechecked items' y_j, laid out as the ladder entry points read their points.
KERNEL2 k_kzg_neg_g1_copies(const u8* src, u8* dst, size_t n) {
    const size_t i = (size_t)blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    G1Aff g = load_g1(src);
    g.y = fp_store(fp_neg(g.y));
    store_g1(dst + (size_t)96 * i, g);
}

// Minus each of the n G1 records at src (4-byte aligned; the all-zero record stays all-zero), a lane per record: the key records -[tau^i] G
// over which a cell batch runs the ladders of its folded coefficients (blsmi 0.22: rlc_host.hpp, cell_core).
KERNEL2 k_kzg_neg_g1_records(const u8* src, u8* dst, size_t n) {
    const size_t i = (size_t)blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    G1Aff g = load_g1(src + (size_t)96 * i);
    g.y = fp_store(fp_neg(g.y));
    store_g1(dst + (size_t)96 * i, g);
}

// The proofs beside the lifted points: record j of src (96 bytes, 4-byte aligned) to the second half of the 192-byte slot j of dst -- (W_j,
// pi_j) interleaved is the G1 array of the two pairs per item.  A lane per 32-bit word.
KERNEL2 k_kzg_place_proofs(const u32* src, u32* dst, size_t n) {
    const size_t t = (size_t)blockIdx.x * WG + threadIdx.x;
    if (t >= 24 * n) return;
    const size_t j = t / 24;
    dst[48 * j + 24 + (t - 24 * j)] = src[t];
}

// The two pairs of every item a KZG batch rechecks, dense, for blsmi_pairing_product_batch's own path: item t (dense) is opening items[t] = j,
// and its pairs are (P_t, H), (pi_j, -tau H) -- P: the dense points C_j + z_j pi_j - y_j G with their infinity bytes; wp: (W_j, pi_j)
// interleaved; tab: H, -tau H.  Sixteen lanes per pair, 16-byte pieces (lanes 0..5 the G1 record, 0..11 the G2 record), the flag byte of the
// pair -- bit 0: the G1 point is infinite, bit 1: the G2 record is all-zero -- from the records themselves.  Every buffer is 16-byte aligned;
// no lane writes beyond pair 2 nre - 1.
KERNEL2 k_kzg_recheck_pairs(const uint4* P, const u8* P_inf, const uint4* wp, const uint4* tab, const u32* items, size_t m, uint4* g1, uint4* g2, u8* flags, size_t nre) {
    const u32 l = threadIdx.x & 15;
    const size_t p = (size_t)blockIdx.x * (WG / 16) + (threadIdx.x >> 4);
    const size_t pp = p < 2 * nre ? p : 2 * nre - 1;
    const size_t t = pp >> 1; const u32 q = (u32)(pp & 1);
    const size_t j = items[t];
    const uint4* a = q == 0 ? P + 6 * t : wp + 12 * j + 6;
    const uint4* b = tab + 12 * q;
    uint4 x = make_uint4(0, 0, 0, 0), y = make_uint4(0, 0, 0, 0);
    if (j < m && l < 6) x = a[l];
    if (j < m && l < 12) y = b[l];
    u32 ax = x.x | x.y | x.z | x.w, ay = y.x | y.y | y.z | y.w;
    ax |= __shfl_xor(ax, 1); ax |= __shfl_xor(ax, 2); ax |= __shfl_xor(ax, 4); ax |= __shfl_xor(ax, 8);
    ay |= __shfl_xor(ay, 1); ay |= __shfl_xor(ay, 2); ay |= __shfl_xor(ay, 4); ay |= __shfl_xor(ay, 8);
    if (p >= 2 * nre) return;
    if (l < 6) g1[6 * p + l] = x;
    if (l < 12) g2[12 * p + l] = y;
    if (l == 0) flags[p] = (u8)(((ax == 0 || (q == 0 && P_inf[t])) ? 1 : 0) | (ay == 0 ? 2 : 0));
}
