// k_fe_pair.hip -- the final-exponentiation kernels of the lane-pair layout (pair_kernels.inc: k_final_exp_pair, k_final_exp_is_one_pair),
// a translation unit of their own because they are compiled with the multiply cores as ASSEMBLY BLOBS behind inline-asm statements
// (BLSMI_ASM_CORES: core_asm.inc, gen_core_asm.py) instead of out-of-line functions: every compiled function begins with
// s_waitcnt vmcnt(0), which drains the caller's scratch stores at each of the ~5 000 products of a final exponentiation; an asm statement
// does not.  Same-box A/B: k_final_exp_pair 11.39 -> 10.93 ms.  The Miller-loop kernels keep the function cores (9.46 -> 9.53 ms with blobs).
#define BLSMI_ASM_CORES
#include "pairing.cuh"
#include "device_io.cuh"

#define BLSMI_PAIR_FE_ONLY
#include "pair_kernels.inc"

// unit-level access (blsmi_debug_op, BLSMI_OP_LANE_PAIR | BLSMI_OP_FQ12_FINAL_EXP): pairing.go:79-129 on k_debug_pairl's 12-Fq records,
// through the same assembly-blob cores as k_final_exp_pair
KERNEL_PAIR k_debug_final_exp_pair(const u64* a, u64* out, size_t n) {
    const int par = threadIdx.x & 1;
    const size_t t0 = (size_t)blockIdx.x * PT + (threadIdx.x >> 1);
    const size_t t = t0 < n ? t0 : n - 1;                                 // both lanes of a pair stay active (DPP partner exchange)
    P2::Fp12S f;
    FpS* c = reinterpret_cast<FpS*>(&f);
    for (int j = 0; j < 6; j++) c[j] = load_m384(a + (size_t)6 * (12 * t + 2 * j + par));
    P2::final_exponentiation(f);
    if (t0 < n)
        for (int j = 0; j < 6; j++) store_m384(out + (size_t)6 * (12 * t + 2 * j + par), c[j]);
}
