// sha256_fs.h -- the Fiat-Shamir challenge of a KZG blob proof (blsmi 0.23: blsmi_kzg_blob_challenge_batch*, k_kzg_fs.hip): where every
// word of the hashed message comes from, and the digest's reduction mod r.  Plain inline C++ with no HIP types, as fr.h, whose qualifier
// FR_FOLD_FN and whose reduction it uses: the kernels include it, and tests/native/sha256_fs.cc runs it natively.
//     z = SHA-256(D) mod r,        D = "FSBLOBVERIFY_V1_" || N as 16 big-endian bytes || the blob, 32 N bytes || the commitment, 48 bytes
// with N = 2^log2n, log2n <= 16.  D is 32 N + 80 bytes; with the padding (0x80, zeros, the bit length as 8 big-endian bytes) that is
// N / 2 + 2 blocks of 64 bytes for N >= 2 and 2 blocks for N = 1:
//     block 0             the 32 bytes of the prefix and N, then value 0 of the blob
//     block 1 .. N/2 - 1  64 bytes of the blob from its offset 64 i - 32 on: the blob sits 32 bytes off the block grid
//     block N/2           the blob's last value, then the commitment's bytes 0 .. 31
//     block N/2 + 1       the commitment's bytes 32 .. 47, 0x80, zeros, the bit length
//     N = 1               block 0 as above; block 1 the 48 bytes of the commitment, 0x80, zeros, the bit length
// Every boundary (32, 32 + 32 N, 32 N + 80) is a multiple of four, so each 32-bit word of a block comes whole from one place.
#pragma once
#include "fr.h"

namespace blsmi_fs {

constexpr unsigned MAX_LOG2N = 16;
// where a word comes from: FS_CONST: v IS the word; FS_BLOB / FS_COMM: the four bytes at offset v of the blob / the commitment, big-endian
constexpr uint32_t FS_CONST = 0, FS_BLOB = 1, FS_COMM = 2;
struct Word { uint32_t src, v; };

FR_FOLD_FN uint32_t blocks(unsigned log2n) { return log2n == 0 ? 2u : ((uint32_t)1 << (log2n - 1)) + 2u; }
// word w (0 .. 15) of block i (0 .. blocks - 1).  All offsets stay below 2^21 + 2^8 and the bit length below 2^25.
FR_FOLD_FN Word word(unsigned log2n, uint32_t i, uint32_t w) {
    const uint32_t n = (uint32_t)1 << log2n, blob_end = 32 + 32 * n, len = blob_end + 48;
    const uint32_t o = 64 * i + 4 * w, last = 64 * blocks(log2n) - 4;
    Word r;
    r.src = FS_CONST; r.v = 0;
    if (o < 16) r.v = o == 0 ? 0x4653424cu : o == 4 ? 0x4f425645u : o == 8 ? 0x52494659u : 0x5f56315fu;   // "FSBL" "OBVE" "RIFY" "_V1_"
    else if (o < 32) r.v = o == 28 ? n : 0;                                      // N as 16 big-endian bytes: N < 2^32
    else if (o < blob_end) { r.src = FS_BLOB; r.v = o - 32; }
    else if (o < len) { r.src = FS_COMM; r.v = o - blob_end; }
    else if (o == len) r.v = 0x80000000u;
    else if (o == last) r.v = len * 8;                                           // the bit length's low word; its high word is 0
    return r;
}
// does block i lie in the blob with all of its 64 bytes?  They are then the blob's bytes 64 i - 32 .. 64 i + 31.
FR_FOLD_FN bool whole_in_blob(unsigned log2n, uint32_t i) { return log2n >= 2 && i >= 1 && i < ((uint32_t)1 << (log2n - 1)); }

// the digest h (h[0] the most significant word) as an integer mod r: eight little-endian words, fully reduced.  r < 2^255 and
// 2^256 - 1 < 3 r: the digest can be >= r and >= 2 r, so up to two conditional subtractions.
FR_FOLD_FN void digest_to_scalar(const uint32_t h[8], uint32_t v[8]) {
    for (int k = 0; k < 8; k++) v[k] = h[7 - k];
    blsmi_fr::reduce_any(v);
}

}  // namespace blsmi_fs
