// k_check.hip -- batch point validation (blsmi 0.14): IsOnCurve (g1.go:93-105, g2.go:118-130) and IsInCorrectSubgroupAssumingOnCurve
// (g1.go:137-141, g2.go:293-295) of n points AS THEY ARRIVE -- affine wire records or the reference's in-memory Jacobian records -- one
// status byte per point: 0 good, 1 infinity, 3 not on the curve, 4 on the curve but outside the prime-order subgroup (3 and 4 are the
// error codes of the decompression kernels, k_wire.hip).  Nothing is inverted and no root is taken: the curve equation is tested on the
// coordinates that came (Jacobian: Y^2 == X^3 + b Z^6) and the subgroup verdict is the infinity flag of [x^2] P + phi(P) (G1) or
// [|x|] P + psi(P) (G2), the endomorphisms acting on the Jacobian triple (subgroup.cuh).  check: 0 the curve equation only, 1 the
// endomorphism test, 2 the reference's r * P walk.  Every lane computes every verdict and the status is selected at the end: a record is
// judged in the order infinity, curve, subgroup, so the "assuming on curve" predicate is never consulted for a point off the curve.
#include "hash.cuh"
#include "device_io.cuh"
#include "subgroup.cuh"

template <class P> BLSMI_DEV bool subgroup_verdict(const P& p, int check) { return check == 2 ? in_subgroup_by_order(p) : check ? in_subgroup(p) : true; }
template <class P, class F> BLSMI_DEV u8 point_status(const P& p, const F& b, int check) {
    const bool curve = on_curve(p, b);
    const bool sub = subgroup_verdict(p, check);
    return p.inf ? BLSMI_POINT_INFINITY : !curve ? BLSMI_POINT_NOT_ON_CURVE : !sub ? BLSMI_POINT_NOT_IN_SUBGROUP : BLSMI_POINT_OK;
}
// ---- one lane per point --------------------------------------------------------------------------------------------------------------
// A coordinate that is not below q is read as every loader reads it (fp_from_words, load_m384_checked: as 0) and the point is judged as that.
KERNEL2 k_g1_check(const u8* pts, const u8* in_inf, int check, u8* status, size_t n) {
    const size_t t = (size_t)blockIdx.x * WG + threadIdx.x;
    const size_t tt = t < n ? t : n - 1;
    G1Aff a = load_g1(pts + 96 * tt);
    if (in_inf && in_inf[tt]) a.inf = -1;
    const u8 st = point_status(a, FpS(C_B), check);
    if (t < n) status[t] = st;
}
KERNEL2 k_g1_check_jac(const u64* pts, int check, u8* status, size_t n) {
    const size_t t = (size_t)blockIdx.x * WG + threadIdx.x;
    const size_t tt = t < n ? t : n - 1;
    const u8 st = point_status(load_jac_m384<FpS>(pts + 18 * tt), FpS(C_B), check);
    if (t < n) status[t] = st;
}
KERNEL k_g2_check(const u8* pts, const u8* in_inf, int check, u8* status, size_t n) {
    const size_t t = (size_t)blockIdx.x * WG + threadIdx.x;
    const size_t tt = t < n ? t : n - 1;
    G2Aff a = load_g2(pts + 192 * tt);
    if (in_inf && in_inf[tt]) a.inf = -1;
    const u8 st = point_status(a, Fp2S(C_B2), check);
    if (t < n) status[t] = st;
}
KERNEL k_g2_check_jac(const u64* pts, int check, u8* status, size_t n) {
    const size_t t = (size_t)blockIdx.x * WG + threadIdx.x;
    const size_t tt = t < n ? t : n - 1;
    const u8 st = point_status(load_jac_m384<Fp2S>(pts + 36 * tt), Fp2S(C_B2), check);
    if (t < n) status[t] = st;
}

// ---- G2 with a lane pair per point (pair_field.cuh: one Fq2 coefficient per lane, two waves per SIMD) ---------------------------------
#include "pair_field.cuh"
namespace P2 = blsmi::pairl;
#include "pair_point_io.inc"
namespace blsmi {
namespace pairl {
BLSMI_DEV G2JacP psi_jac(const G2JacP& g) {                                // hash.cuh: psi_jac, each lane on its own coefficient
    G2JacP r;
    r.x = fp2_store(fp2_mul(BLSMI_FP2_K(C_PSI_CX), fp2_conj(g.x)));
    r.y = fp2_store(fp2_mul(BLSMI_FP2_K(C_PSI_CY), fp2_conj(g.y)));
    r.z = fp2_store(fp2_conj(g.z));
    r.inf = g.inf;
    return r;
}
BLSMI_DEV bool in_subgroup(const G2JacP& p) { return jac_add(jac_mul_u64_public(p, BLSMI_X_ABS), psi_jac(p)).inf != 0; }
BLSMI_DEV bool in_subgroup(const G2AffP& p) { return jac_add(aff_mul_u64_public(p, BLSMI_X_ABS), psi_jac(to_jac(p))).inf != 0; }   // (mixed additions in the ladder)
}  // namespace pairl
}  // namespace blsmi
// the in-memory record x.c0 x.c1 y.c0 y.c1 z.c0 z.c1 (6 LE u64 each): lane `par` takes coefficient c_par of each coordinate; z == 0 <=> both are
BLSMI_DEV P2::G2JacP pair_load_jac_m384(const u64* rec, int par) {
    u32 nz_xy = 0, nz_z = 0, diff = 0;
    P2::G2JacP j;
    j.x = P2::wrap(load_m384_checked(rec + 6 * (0 + par), nz_xy, diff, nullptr));
    j.y = P2::wrap(load_m384_checked(rec + 6 * (2 + par), nz_xy, diff, nullptr));
    j.z = P2::wrap(load_m384_checked(rec + 6 * (4 + par), nz_z, diff, nullptr));
    nz_z |= (u32)__shfl_xor((int)nz_z, 1);
    j.inf = nz_z ? 0 : -1;
    return j;
}
// (both lanes of a pair stay active to the end: the cross-lane moves of the Fq2 products read the partner)
__global__ void __launch_bounds__(WG, 2) k_g2_check_pair(const u8* pts, const u8* in_inf, int check, u8* status, size_t n) {
    const int par = threadIdx.x & 1;
    const size_t t = (size_t)blockIdx.x * (WG / 2) + (threadIdx.x >> 1);
    const size_t tt = t < n ? t : n - 1;
    P2::G2AffP a = pair_load_g2(pts + 192 * tt, par);
    if (in_inf && in_inf[tt]) a.inf = -1;
    const u8 st = point_status(a, P2::fp2_pair_const(C_B2), check);
    if (t < n && !par) status[t] = st;
}
__global__ void __launch_bounds__(WG, 2) k_g2_check_jac_pair(const u64* pts, int check, u8* status, size_t n) {
    const int par = threadIdx.x & 1;
    const size_t t = (size_t)blockIdx.x * (WG / 2) + (threadIdx.x >> 1);
    const size_t tt = t < n ? t : n - 1;
    const u8 st = point_status(pair_load_jac_m384(pts + 36 * tt, par), P2::fp2_pair_const(C_B2), check);
    if (t < n && !par) status[t] = st;
}
