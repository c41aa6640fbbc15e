// subgroup.cuh -- the curve equation and the prime-order-subgroup predicates, one point per lane, for the units that judge points:
// k_wire.hip (decompression: affine points it has just built) and k_check.hip (validation of points as they arrive, affine or Jacobian).
// Include after hash.cuh (psi, psi_jac).
#pragma once
#include "hash.cuh"

namespace blsmi {
// IsInCorrectSubgroupAssumingOnCurve (g1.go:137-141, g2.go:293-295) tests r * P == infinity with a 255-bit
// double-and-add.  The same predicate, for a point ON the curve, through the curve's endomorphisms:
//   G1: phi(x, y) = (beta x, y) satisfies phi^2 + phi + 1 = 0; phi(P) = [-x^2] P implies (x^4 - x^2 + 1) P = r P = 0,
//       and on G1 phi acts as that eigenvalue: two 64-bit multiplications instead of one 255-bit one.
//   G2: psi (untwist-Frobenius-twist) satisfies psi^2 - t psi + q = 0 with t = x + 1; psi(P) = [x] P implies
//       (q - x) P = (h1 r) P = 0, so the order of P divides r gcd(h1, h2) = r (the cofactors are coprime), and on
//       G2 psi acts as x: one 64-bit multiplication.
// The slow form is kept (in_subgroup_by_order) and the two are compared on curve points inside and outside
// the subgroup by tests/test_gpu_verify.py::test_wire_format.
template <class F> BLSMI_DEV bool in_subgroup_by_order(const Aff<F>& p) {
    Jac<F> res = to_jac(p);
    for (int i = BLSMI_R_ORDER_BITS - 2; i >= 0; i--) {
        res = jac_double(res);
        if ((C_R_ORDER[i >> 5] >> (i & 31)) & 1) res = jac_add_affine(res, p);
    }
    return res.inf != 0;
}
BLSMI_DEV bool in_subgroup(const G1Aff& p) {                             // [x^2] P + phi(P) == infinity
    const G1Jac j = jac_mul_u64_public(aff_mul_u64_public(p, BLSMI_X_ABS), BLSMI_X_ABS);
    G1Aff ph; ph.x = fp_store(fp_mul(p.x, C_BETA)); ph.y = p.y; ph.inf = 0;
    return jac_add_affine(j, ph).inf != 0;
}
BLSMI_DEV bool in_subgroup(const G2Aff& p) {                             // [|x|] P + psi(P) == infinity  (x < 0)
    const G2Jac j = aff_mul_u64_public(p, BLSMI_X_ABS);
    G2Aff ps; psi(ps, p);
    return jac_add_affine(j, ps).inf != 0;
}

// ---- the same predicates on a Jacobian point (X, Y, Z), x = X / Z^2, y = Y / Z^3, without leaving its coordinates ------------
// Both endomorphisms are monomial maps, so they act on the Jacobian triple directly: phi(X, Y, Z) = (beta X, Y, Z) (beta x = beta X / Z^2),
// psi(X, Y, Z) = (Cx conj X, Cy conj Y, conj Z) (hash.cuh: psi_jac; conj is a field automorphism).  The ladders take a Jacobian base
// (general additions) and the last step is a general addition with its equal-point and opposite-point branches: the verdict is the
// infinity flag of a sum, which no division is needed to read.
template <class F> BLSMI_DEV bool in_subgroup_by_order(const Jac<F>& p) {
    Jac<F> res = p;
#pragma unroll 1
    for (int i = BLSMI_R_ORDER_BITS - 2; i >= 0; i--) {                   // (inlined bodies, one copy each, as jac_mul_u64_public: no callee frame in scratch)
        res = jac_double_i(res);
        if ((C_R_ORDER[i >> 5] >> (i & 31)) & 1) res = jac_add_i(res, p);
    }
    return res.inf != 0;
}
BLSMI_DEV bool in_subgroup(const G1Jac& p) {
    const G1Jac j = jac_mul_u64_public(jac_mul_u64_public(p, BLSMI_X_ABS), BLSMI_X_ABS);
    G1Jac ph = p; ph.x = fp_store(fp_mul(p.x, C_BETA));
    return jac_add(j, ph).inf != 0;
}
BLSMI_DEV bool in_subgroup(const G2Jac& p) { return jac_add(jac_mul_u64_public(p, BLSMI_X_ABS), psi_jac(p)).inf != 0; }

// ---- the curve equation on the coordinates as they arrive (g1.go:93-105, g2.go:118-130: y^2 == x^3 + b) ------------------------
// Jacobian: Y^2 / Z^6 == X^3 / Z^6 + b  <=>  Y^2 == X^3 + b Z^6 (Z != 0).  b: the curve's coefficient in the field layout of F.
template <class F> BLSMI_DEV bool on_curve(const Aff<F>& p, const F& b) {
    const F lhs = f_store(f_sqr(p.y));
    const F rhs = f_store(f_add(f_mul(f_store(f_sqr(p.x)), p.x), b));
    return f_is_zero(f_store(f_sub(lhs, rhs)));
}
template <class F> BLSMI_DEV bool on_curve(const Jac<F>& p, const F& b) {
    const F z2 = f_store(f_sqr(p.z));
    const F z6 = f_store(f_mul(f_store(f_sqr(z2)), z2));
    const F lhs = f_store(f_sqr(p.y));
    const F rhs = f_store(f_add(f_mul(f_store(f_sqr(p.x)), p.x), f_store(f_mul(b, z6))));
    return f_is_zero(f_store(f_sub(lhs, rhs)));
}
}  // namespace blsmi
