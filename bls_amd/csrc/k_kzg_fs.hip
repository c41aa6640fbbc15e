// k_kzg_fs.hip -- the Fiat-Shamir challenge of KZG blob proofs on the device (blsmi 0.23: blsmi_kzg_blob_challenge_batch*, and through it
// blsmi_kzg_verify_blob_batch_wire*, rlc_host.hpp): z_j = SHA-256(D_j) mod r over the blob and the compressed commitment as they lie, and
// the two byte kernels that give the wire call its status and its verdicts.  Which bytes make which word of which block, and the digest's
// reduction, are sha256_fs.h, which runs natively as well; the compression function is hash.cuh's.
//   k_kzg_fs_lane    one lane per blob, 64 blobs per wave; a lane walks its N / 2 + 2 blocks
//   k_kzg_fs_split   a workgroup of two waves per 64 blobs: wave 1 loads block i + 1 and writes W[t] + K[t], t = 0 .. 63, into one half of a
//                    double-buffered LDS array while wave 0 runs the 64 rounds of block i from the other half; one barrier per block
// A block that lies whole in the blob (all but three of them) is 64 contiguous bytes: four 16-byte loads when the buffer is 16-byte aligned,
// sixteen words otherwise; the other blocks are built word by word.  Lanes at or beyond m hash item m - 1 again and store nothing.
// No atomics, plain stores.  k_kzg_fs_lane hands sha256_block (not inlined) its two arrays through 112 bytes of scratch a lane, as every caller of
// that function does; k_kzg_fs_split, whose rounds are its own, uses none.
#include "hash.cuh"
#include "sha256_fs.h"

using namespace blsmi;

namespace {
// the sixteen words of block i of one item, in SHA's big-endian order.  blob, comm: 4-byte aligned; al: blob is 16-byte aligned
__device__ inline void fs_load_block(const u8* blob, const u8* comm, u32 log2n, u32 i, bool al, u32 w[16]) {
    if (blsmi_fs::whole_in_blob(log2n, i)) {
        const u8* p = blob + ((size_t)64 * i - 32);
        if (al) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint4 v = reinterpret_cast<const uint4*>(p)[q];
                w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 16; k++) w[k] = reinterpret_cast<const u32*>(p)[k];
        }
#pragma unroll
        for (int k = 0; k < 16; k++) w[k] = __builtin_bswap32(w[k]);
    } else {
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const blsmi_fs::Word s = blsmi_fs::word(log2n, i, (u32)k);
            w[k] = s.v;
            if (s.src != blsmi_fs::FS_CONST) w[k] = __builtin_bswap32(*reinterpret_cast<const u32*>((s.src == blsmi_fs::FS_BLOB ? blob : comm) + s.v));
        }
    }
}
// the digest mod r as 32 big-endian bytes at p (4-byte aligned)
__device__ inline void fs_store(u8* p, const u32 h[8]) {
    u32 v[8];
    blsmi_fs::digest_to_scalar(h, v);
    u32* q = reinterpret_cast<u32*>(p);
#pragma unroll
    for (int k = 0; k < 8; k++) q[k] = __builtin_bswap32(v[7 - k]);
}
}  // namespace

#define FS_WG 64
#define FS_SPLIT_WG 128

// polys: m blobs of N = 2^log2n values of 32 bytes, comm: m compressed commitments of 48 bytes, z: m challenges of 32 big-endian bytes, fully
// reduced; every buffer 4-byte aligned.  Nothing is decoded: the bytes are hashed as they lie.
__global__ void __launch_bounds__(FS_WG) k_kzg_fs_lane(const u8* polys, u32 log2n, const u8* comm, u8* z, size_t m) {
    const size_t j = (size_t)blockIdx.x * FS_WG + threadIdx.x, jj = j < m ? j : m - 1;
    const u8* blob = polys + (jj << (log2n + 5));
    const u8* c = comm + 48 * jj;
    const bool al = (reinterpret_cast<uintptr_t>(polys) & 15) == 0;
    const u32 nb = blsmi_fs::blocks(log2n);
    u32 h[8];
    sha256_init(h);
    for (u32 i = 0; i < nb; i++) {
        u32 w[16];
        fs_load_block(blob, c, log2n, i, al, w);
        sha256_block(h, w);
    }
    if (j < m) fs_store(z + 32 * j, h);
}

// The same with the message schedule on a wave of its own.  LDS: two halves of 64 x 64 words, 16 KB each; word t of lane l at
// ((t / 4) * 64 + l) * 4 + t % 4 -- a lane's four consecutive words are one 16-byte slot and consecutive lanes take consecutive slots, so
// that wave 1's sixteen 16-byte stores and wave 0's sixteen 16-byte loads per block are free of bank conflicts.  Step s: wave 1 fills half
// s % 2 with block s (s < nb), wave 0 runs block s - 1 from the other half (s >= 1); one barrier ends the step, nb + 1 in all, and every
// wave reaches every one.  Wave 0 issues no global load and no schedule arithmetic.
__global__ void __launch_bounds__(FS_SPLIT_WG) k_kzg_fs_split(const u8* polys, u32 log2n, const u8* comm, u8* z, size_t m) {
    __shared__ uint4 lds[2][16][64];
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t j = (size_t)blockIdx.x * 64 + lane, jj = j < m ? j : m - 1;
    const u8* blob = polys + (jj << (log2n + 5));
    const u8* c = comm + 48 * jj;
    const bool al = (reinterpret_cast<uintptr_t>(polys) & 15) == 0;
    const u32 nb = blsmi_fs::blocks(log2n);
    u32 h[8];
    sha256_init(h);
    for (u32 s = 0; s <= nb; s++) {
        if (wave == 1) {
            if (s < nb) {
                u32 w[16];
                fs_load_block(blob, c, log2n, s, al, w);
#pragma unroll
                for (int t = 0; t < 64; t += 4) {
                    u32 o[4];
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        const int i = t + e;
                        if (i >= 16) {
                            const u32 w15 = w[(i - 15) & 15], w2 = w[(i - 2) & 15];
                            const u32 s0 = rotr(w15, 7) ^ rotr(w15, 18) ^ (w15 >> 3), s1 = rotr(w2, 17) ^ rotr(w2, 19) ^ (w2 >> 10);
                            w[i & 15] = w[i & 15] + s0 + w[(i - 7) & 15] + s1;
                        }
                        o[e] = w[i & 15] + SHA_K[i];
                    }
                    lds[s & 1][t >> 2][lane] = make_uint4(o[0], o[1], o[2], o[3]);
                }
            }
        } else if (s >= 1) {
            u32 a = h[0], b = h[1], cc = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll
            for (int t = 0; t < 64; t += 4) {
                const uint4 q = lds[(s - 1) & 1][t >> 2][lane];
                const u32 wk[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const u32 t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + wk[k];
                    const u32 t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & cc) ^ (b & cc));
                    hh = g; g = f; f = e; e = d + t1; d = cc; cc = b; b = a; a = t1 + t2;
                }
            }
            h[0] += a; h[1] += b; h[2] += cc; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
        }
        __syncthreads();
    }
    if (wave == 0 && j < m) fs_store(z + 32 * j, h);
}

// ---- the wire call's status and verdicts ---------------------------------------------------------------------------------------------------
// err: the 2 m error codes of the decompression, the m commitments' first, then the m proofs'; noncanon: m flags of the evaluation.
// status[j] = errC | errPi << 3 | noncanon << 6.  An item with status != 0 is cleared to the item that holds trivially -- both records all
// zero (infinity), y = 0 --, so that it cannot fail its block; k_kzg_wire_verdicts takes its verdict back afterwards.  pts: the 2 m affine
// records in the order of err; y: m scalars; a lane per item.
__global__ void __launch_bounds__(FS_WG) k_kzg_wire_status(const u8* err, const u8* noncanon, u8* status, u8* pts, u8* y, size_t m) {
    const size_t j = (size_t)blockIdx.x * FS_WG + threadIdx.x;
    if (j >= m) return;
    const u8 st = (u8)(err[j] | err[m + j] << 3 | (noncanon[j] ? 0x40 : 0));
    status[j] = st;
    if (st == 0) return;
    u32* c = reinterpret_cast<u32*>(pts + 96 * j);
    u32* p = reinterpret_cast<u32*>(pts + 96 * (m + j));
    u32* yy = reinterpret_cast<u32*>(y + 32 * j);
    for (int k = 0; k < 24; k++) { c[k] = 0; p[k] = 0; }
    for (int k = 0; k < 8; k++) yy[k] = 0;
}
// ok[j] = 1 exactly when it was 1 and status[j] == 0
__global__ void __launch_bounds__(FS_WG) k_kzg_wire_verdicts(const u8* status, u8* ok, size_t m) {
    const size_t j = (size_t)blockIdx.x * FS_WG + threadIdx.x;
    if (j < m && status[j] != 0) ok[j] = 0;
}
