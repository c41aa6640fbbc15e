// k_fr_eval.hip -- the scalar field proper on the device (blsmi 0.21): products and inverses mod r, a lane per element
// (blsmi_fr_mul_batch*, blsmi_fr_inv_batch*), and the evaluation of polynomials given by their values over the 2^k-th roots of unity
// (blsmi_fr_eval_batch*, and through it blsmi_kzg_verify_blob_batch*, rlc_host.hpp).  The arithmetic is fr.h, which runs natively as well.
//     p(z) = (z^N - 1) / N * sum_i f_i w_i / (z - w_i)                              (the barycentric formula; w_i the root at position i)
// One workgroup of 256 lanes per polynomial, lane l the positions i = l, l + 256, ...; ONE inversion per polynomial, between two launches:
//   k_fr_bary_prod   D_j = prod_i d_i, d_i = z_j - w_i (a zero d_i -- z_j is the root at position i -- recorded in hit[j] and replaced by one)
//   k_fr_inv         D_j^-1
//   k_fr_bary_sum    the sum, from the lanes' shares as fractions and the inverses of the lanes' denominators out of D_j^-1
// Scalars cross between kernels as the library's 32 big-endian bytes.  No atomics; LDS is one tree of 512 elements (16 KB).
#include <hip/hip_runtime.h>
#include "fr.h"
#include "fr_dev_io.cuh"                                                       // scalars and table elements in device memory

#define FR_WG 256
#define FR_NO_HIT 0xffffffffu

namespace {
// ---- the tree over the 256 lanes, in LDS: 512 slots word-major (word k of slot s at k * 512 + s), the root in slot 1, the children of node
// n in slots 2 n and 2 n + 1, the lanes' leaves in slots 256 + l.  Slot 0 is not used.
__device__ inline Fr lds_get(const u32* lds, u32 slot) {
    Fr o;
#pragma unroll
    for (int k = 0; k < 8; k++) o.w[k] = lds[k * 512 + slot];
    return o;
}
__device__ inline void lds_put(u32* lds, u32 slot, const Fr& v) {
#pragma unroll
    for (int k = 0; k < 8; k++) lds[k * 512 + slot] = v.w[k];
}
// up: every node the product of its children; the root ends as the product of the 256 leaves.  (A level reads the level below and writes
// its own: no lane reads what another writes between two barriers.)
__device__ inline void tree_up(u32* lds, u32 l, const Fr& leaf) {
    lds_put(lds, FR_WG + l, leaf);
    __syncthreads();
    for (u32 h = FR_WG / 2; h >= 1; h >>= 1) {
        if (l < h) lds_put(lds, h + l, blsmi_fr::mul(lds_get(lds, 2 * (h + l)), lds_get(lds, 2 * (h + l) + 1)));
        __syncthreads();
    }
}
// down, the root's slot holding the INVERSE of the product: a node's inverse times its right child's product is the left child's inverse
// and the other way round (Montgomery's trick over the tree, two products per node); the leaves end as the inverses of the lanes' leaves.
// A lane reads its node's slot, written a level before, and its two children's, which it alone overwrites.
__device__ inline void tree_down(u32* lds, u32 l) {
    for (u32 h = 1; h <= FR_WG / 2; h <<= 1) {
        if (l < h) {
            const u32 n = h + l;
            const Fr iv = lds_get(lds, n), lo = lds_get(lds, 2 * n), hi = lds_get(lds, 2 * n + 1);
            lds_put(lds, 2 * n, blsmi_fr::mul(iv, hi));
            lds_put(lds, 2 * n + 1, blsmi_fr::mul(iv, lo));
        }
        __syncthreads();
    }
}
// d = z - w, a zero difference replaced by one; *zero tells
__device__ inline Fr bary_diff(const Fr& z, const Fr& w, bool* zero) {
    const Fr d = blsmi_fr::sub(z, w);
    *zero = blsmi_fr::is_zero(d);
    return *zero ? blsmi_fr::one() : d;
}
}  // namespace

// out[t] = a[t] b[t] mod r, a lane per element; 32 big-endian bytes each, any value taken mod r; every buffer 4-byte aligned.
__global__ void __launch_bounds__(FR_WG) k_fr_mul(const u8* a, const u8* b, u8* out, size_t n) {
    const size_t t = (size_t)blockIdx.x * FR_WG + threadIdx.x;
    if (t >= n) return;
    u32 x[8], y[8], v[8];
    load_scalar4(a + 32 * t, x); load_scalar4(b + 32 * t, y);
    blsmi_fr::mont_mul_words(blsmi_fr::from_words(x).w, y, v);                  // (x R) y / R: the plain product, reduced (fr.h: one factor below r)
    store_scalar4(out + 32 * t, v);
}

// out[t] = a[t]^-1 mod r, and 0 for a[t] = 0 mod r, a lane per element: Fermat's exponent (fr.h).  The one inversion a polynomial's
// evaluation pays, and the kernel of blsmi_fr_inv_batch*.
__global__ void __launch_bounds__(FR_WG) k_fr_inv(const u8* a, u8* out, size_t n) {
    const size_t t = (size_t)blockIdx.x * FR_WG + threadIdx.x;
    if (t >= n) return;
    u32 x[8], v[8];
    load_scalar4(a + 32 * t, x);
    blsmi_fr::to_words(blsmi_fr::inv(blsmi_fr::from_words(x)), v);
    store_scalar4(out + 32 * t, v);
}

// The denominators' product.  tab: the domain of size N = 2^log2n in position order and N^-1 behind it (fr.h: domain_table); z: m points,
// 4-byte aligned.  Workgroup j (and j + gridDim.x, ...) reads only z_j and the table: lane l multiplies its d_i = z_j - w_i, i = l, l + 256,
// ... -- a lane beyond N keeps one -- and the 256 lanes' products meet in the tree.  D[j]: the product as 32 big-endian bytes; hit[j]: the
// position i with z_j = w_i mod r (its d_i counted as one), else 0xffffffff.  The roots are distinct: at most one lane finds one.
__global__ void __launch_bounds__(FR_WG) k_fr_bary_prod(const u8* z, const u32* tab, u32 log2n, u8* D, u32* hit, size_t m) {
    __shared__ u32 lds[8 * 2 * FR_WG];
    __shared__ u32 s_hit;
    const u32 l = threadIdx.x;
    const size_t N = (size_t)1 << log2n;
    for (size_t j = blockIdx.x; j < m; j += gridDim.x) {
        if (l == 0) s_hit = FR_NO_HIT;
        __syncthreads();
        u32 zw[8];
        load_scalar4(z + 32 * j, zw);
        const Fr zt = blsmi_fr::from_words(zw);
        Fr p = blsmi_fr::one();
        for (size_t i = l; i < N; i += FR_WG) {
            bool zero;
            const Fr d = bary_diff(zt, load_table(tab, i), &zero);
            if (zero) s_hit = (u32)i;
            p = blsmi_fr::mul(p, d);
        }
        tree_up(lds, l, p);
        if (l == 0) {
            u32 v[8];
            blsmi_fr::to_words(lds_get(lds, 1), v);
            store_scalar4(D + 32 * j, v);
            hit[j] = s_hit;
        }
    }
}

// The sum.  polys: m polynomials of N values, 32 big-endian bytes each, ANY 256-bit value taken mod r; read as 16-byte pieces when the buffer
// is 16-byte aligned, else byte by byte (the same for the whole grid).  Dinv, hit: what k_fr_bary_prod and k_fr_inv left.  Lane l walks its
// positions once and keeps its share sum f_i w_i / d_i as a fraction num / den, den the product of its d_i:
//     num <- num d_i + (f_i w_i) den,    den <- den d_i                                (four products per value, nothing stored per value)
// -- f_i w_i is ONE Montgomery product of the unreduced f_i by the table's w_i R, so it comes out as the plain value, and every num carries
// that missing factor R to the end.  The lanes' den meet in the tree as in k_fr_bary_prod (its root is D_j again); the tree is walked down
// from D_j^-1 to the inverse of every lane's den; the lanes' num / den meet by halving.  Lane 0 multiplies by (z^N - 1) N^-1 (log2n
// squarings) -- that product, of the sum without its R by a Montgomery form, IS the plain value -- and writes y[j], fully reduced.  Where
// hit[j] names a position the answer is that value mod r, read again, and the general path's result is not used.  noncanon (may be null):
// noncanon[j] = 1 when any of the N values was >= r, else 0.
__global__ void __launch_bounds__(FR_WG) k_fr_bary_sum(const u8* polys, const u8* z, const u32* tab, u32 log2n, const u8* Dinv, const u32* hit, u8* y, u8* noncanon, size_t m) {
    __shared__ u32 lds[8 * 2 * FR_WG];
    __shared__ u32 s_nc;
    const u32 l = threadIdx.x;
    const size_t N = (size_t)1 << log2n;
    const bool al = (reinterpret_cast<uintptr_t>(polys) & 15) == 0;
    for (size_t j = blockIdx.x; j < m; j += gridDim.x) {
        if (l == 0) s_nc = 0;
        __syncthreads();
        u32 zw[8];
        load_scalar4(z + 32 * j, zw);
        const Fr zt = blsmi_fr::from_words(zw);
        const u8* f = polys + j * N * 32;
        Fr num = blsmi_fr::zero(), den = blsmi_fr::one();
        bool nc = false;
        for (size_t i = l; i < N; i += FR_WG) {
            u32 fw[8];
            load_scalar(f + 32 * i, al, fw);
            nc |= !blsmi_fr::is_canonical(fw);
            const Fr w = load_table(tab, i);
            bool zero;
            const Fr d = bary_diff(zt, w, &zero);
            Fr a;
            blsmi_fr::mont_mul_words(fw, w.w, a.w);
            num = blsmi_fr::add(blsmi_fr::mul(num, d), blsmi_fr::mul(a, den));
            den = blsmi_fr::mul(den, d);
        }
        if (nc) s_nc = 1;                                                      // (every writer writes the same value)
        tree_up(lds, l, den);
        if (l == 0) {
            u32 v[8];
            load_scalar4(Dinv + 32 * j, v);
            lds_put(lds, 1, blsmi_fr::from_words(v));
        }
        __syncthreads();
        tree_down(lds, l);
        Fr s = blsmi_fr::mul(num, lds_get(lds, FR_WG + l));
        lds_put(lds, FR_WG + l, s);                                            // (the lane's own leaf, read just above by itself alone)
        __syncthreads();
        for (u32 h = FR_WG / 2; h >= 1; h >>= 1) {
            if (l < h) { s = blsmi_fr::add(s, lds_get(lds, FR_WG + l + h)); lds_put(lds, FR_WG + l, s); }   // (reads leaves >= h, writes its own < h)
            __syncthreads();
        }
        if (l == 0) {
            u32 v[8];
            const u32 at = hit[j];
            if (at != FR_NO_HIT) {
                load_scalar(f + 32 * (size_t)at, al, v);
                blsmi_fr::reduce_any(v);
            } else {
                Fr c = zt;
                for (u32 q = 0; q < log2n; q++) c = blsmi_fr::sqr(c);
                c = blsmi_fr::mul(blsmi_fr::sub(c, blsmi_fr::one()), load_table(tab, N));
                blsmi_fr::mont_mul_words(s.w, c.w, v);
            }
            store_scalar4(y + 32 * j, v);
            if (noncanon) noncanon[j] = (u8)s_nc;
        }
    }
}
