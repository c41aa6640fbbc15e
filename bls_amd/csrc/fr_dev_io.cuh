// fr_dev_io.cuh -- scalars of Fr in device memory, for the kernels over fr.h (k_fr_eval.hip, k_fr_ntt.hip): the library's 32 big-endian
// bytes as eight little-endian words and back, and the elements of a domain table.
#pragma once
#include <hip/hip_runtime.h>
#include "fr.h"

typedef uint8_t u8;
typedef uint32_t u32;
using blsmi_fr::Fr;

namespace {
// ---- scalars in memory ----
// 32 big-endian bytes at p as eight little-endian words: p 4-byte aligned
__device__ inline void load_scalar4(const u8* p, u32 v[8]) {
    const u32* q = reinterpret_cast<const u32*>(p);
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = __builtin_bswap32(q[7 - k]);
}
// ... p 16-byte aligned (al), two 16-byte loads; otherwise byte by byte, whatever the alignment
__device__ inline void load_scalar(const u8* p, bool al, u32 v[8]) {
    if (al) {
        const uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1];
        v[0] = __builtin_bswap32(b.w); v[1] = __builtin_bswap32(b.z); v[2] = __builtin_bswap32(b.y); v[3] = __builtin_bswap32(b.x);
        v[4] = __builtin_bswap32(a.w); v[5] = __builtin_bswap32(a.z); v[6] = __builtin_bswap32(a.y); v[7] = __builtin_bswap32(a.x);
    } else blsmi_fr::load_be32(p, v);
}
__device__ inline void store_scalar4(u8* p, const u32 v[8]) {
    u32* q = reinterpret_cast<u32*>(p);
#pragma unroll
    for (int k = 0; k < 8; k++) q[k] = __builtin_bswap32(v[7 - k]);
}
// element i of a domain table (Montgomery words, 32-byte aligned)
__device__ inline Fr load_table(const u32* tab, size_t i) {
    const uint4 a = reinterpret_cast<const uint4*>(tab + 8 * i)[0], b = reinterpret_cast<const uint4*>(tab + 8 * i)[1];
    Fr o;
    o.w[0] = a.x; o.w[1] = a.y; o.w[2] = a.z; o.w[3] = a.w; o.w[4] = b.x; o.w[5] = b.y; o.w[6] = b.z; o.w[7] = b.w;
    return o;
}
}  // namespace
