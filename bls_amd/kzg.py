"""KZG batches (blsmi 0.20): blsmi_kzg_verify_batch[_jac|_dev|_jac_dev] and the G1 lift blsmi_g1_mul_add_batch[_dev] they are built on,
and the blob batches that evaluate their polynomials first (blsmi 0.21: blsmi_kzg_verify_blob_batch[_jac|_dev|_jac_dev]), and the cell
batches that interpolate their cells over a coset first (blsmi 0.22: blsmi_kzg_verify_cell_batch[_jac|_dev|_jac_dev]), and the Fiat-Shamir
challenge of a blob proof with the blob batches from wire bytes that derive it (blsmi 0.23: blsmi_kzg_blob_challenge_batch[_dev],
blsmi_kzg_verify_blob_batch_wire[_dev]), over the same binder as bls_amd.engine (engine._fn / engine._call: the types come from include/blsmi.h).  Host code only: every computation
happens in the HIP kernels; a missing library or device raises, nothing falls back."""
import ctypes as C

import numpy as np

from . import engine as _e
from . import fr as _fr


def _stride(stride, what):
    stride = int(stride)
    if stride != 0 and (stride < 96 or stride % 4):
        raise ValueError("%s is 0 (one common record) or a multiple of 4 that is at least 96, got %d" % (what, stride))
    return stride


def _strided(x, stride, n, what):
    """n affine G1 records `stride` bytes apart as a byte array of exactly the span they cover"""
    a = _e._u8(x)
    need = stride * (n - 1) + 96 if n else 0
    if a.size != need:
        raise ValueError("%s: expected %d bytes (%d records %d apart), got %d" % (what, need, n, stride, a.size))
    return a


def g1_mul_add_batch(a, b, scalars, n, a_stride=96, b_stride=96):
    """blsmi_g1_mul_add_batch -> (out (n, 96) uint8, inf (n,) bool): out[j] = A_j + (k_j mod r) * B_j.  a, b: affine records a_stride /
    b_stride bytes apart (0: one common record), exactly the bytes the n records span; scalars: n values of 32 big-endian bytes, any
    256-bit value.  Every B_j lies in the prime-order subgroup (see engine.g1_mul_batch); A_j may be any curve point."""
    n = int(n)
    if n < 0:
        raise ValueError("n is a number of items, got %d" % n)
    a_stride, b_stride = _stride(a_stride, "a_stride"), _stride(b_stride, "b_stride")
    pa, pb = _strided(a, a_stride, n, "a"), _strided(b, b_stride, n, "b")
    k = _e._u8(scalars, 32 * n)
    out = np.zeros((n, 96), dtype=np.uint8)
    inf = np.zeros(n, dtype=np.uint8)
    _e._call("blsmi_g1_mul_add_batch", _e._p8(pa), a_stride, _e._p8(pb), b_stride, _e._p8(k), _e._p8(out.reshape(-1)), _e._p8(inf), n)
    return out, inf.astype(bool)


def g1_mul_add_batch_dev(d_a, a_stride, d_b, b_stride, d_scalars, d_out, d_out_inf, n, stream=0):
    """device-pointer form (ints); the n dense records are in d_out and the infinity bytes in d_out_inf when the call returns"""
    _e._call("blsmi_g1_mul_add_batch_dev", d_a, _stride(a_stride, "a_stride"), d_b, _stride(b_stride, "b_stride"), d_scalars, d_out, d_out_inf, n, stream)


def _verify(name, jac, srs_g1, srs_g2, commitments, proofs, z, y, scalars, block):
    pb, qb = (144, 288) if jac else (96, 192)
    g, h = _e._u8(srs_g1, pb), _e._u8(srs_g2, 2 * qb)
    c, p = _e._u8(commitments), _e._u8(proofs)
    if c.size % pb or p.size != c.size:
        raise ValueError("expected m*%d bytes of C_j and as many of pi_j, got %d and %d" % (pb, c.size, p.size))
    m = c.size // pb
    zz, yy = _e._u8(z, 32 * m), _e._u8(y, 32 * m)
    pr = _e._scalars(scalars, m)
    block = _e._block(block)
    ok = np.zeros(max(1, m), dtype=np.uint8)
    comb, nre = C.c_int(0), C.c_size_t(0)
    g, h, c, p = (_e._recs(v, v.size, jac) for v in (g, h, c, p))
    _e._call(name, g, h, c, p, _e._p8(zz), _e._p8(yy), m, pr, block, _e._p8(ok), C.byref(comb), C.byref(nre))
    return ok[:m].copy(), comb.value, nre.value


def verify_batch(srs_g1, srs_g2, commitments, proofs, z, y, scalars=None, block=0):
    """blsmi_kzg_verify_batch -> (ok (m,) uint8, combined, rechecked): m KZG openings under one key.  srs_g1: G (96 bytes); srs_g2: H, tau H
    (192 each); commitments: C_j; proofs: pi_j (96 each); z, y: m scalars of 32 big-endian bytes each, any value taken mod r.  ok[j] is the
    verdict of engine.pairing_product_batch on (C_j + z_j pi_j - y_j G, H), (pi_j, -tau H); scalars and block as
    engine.pairing_product_batch_rlc_locate."""
    return _verify("blsmi_kzg_verify_batch", False, srs_g1, srs_g2, commitments, proofs, z, y, scalars, block)


def verify_batch_jac(srs_g1_jac, srs_g2_jac, commitments_jac, proofs_jac, z, y, scalars=None, block=0):
    """the same over in-memory points (144 / 288 bytes each, z == 0: infinity)"""
    return _verify("blsmi_kzg_verify_batch_jac", True, srs_g1_jac, srs_g2_jac, commitments_jac, proofs_jac, z, y, scalars, block)


def _verify_dev(name, d_srs_g1, d_srs_g2, d_commitments, d_proofs, d_z, d_y, m, d_ok, scalars, block, stream):
    pr = _e._scalars(scalars, m)
    comb, nre = C.c_int(0), C.c_size_t(0)
    _e._call(name, d_srs_g1, d_srs_g2, d_commitments, d_proofs, d_z, d_y, m, pr, _e._block(block), d_ok, C.byref(comb), C.byref(nre), stream)
    return comb.value, nre.value


def verify_batch_dev(d_srs_g1, d_srs_g2, d_commitments, d_proofs, d_z, d_y, m, d_ok, scalars=None, block=0, stream=0):
    """device-pointer form (ints) over affine records; the m verdict bytes are in d_ok when the call returns; scalars stay on the host.
    -> (combined, rechecked)"""
    return _verify_dev("blsmi_kzg_verify_batch_dev", d_srs_g1, d_srs_g2, d_commitments, d_proofs, d_z, d_y, m, d_ok, scalars, block, stream)


def verify_batch_jac_dev(d_srs_g1_jac, d_srs_g2_jac, d_commitments_jac, d_proofs_jac, d_z, d_y, m, d_ok, scalars=None, block=0, stream=0):
    """device-pointer form over in-memory points -> (combined, rechecked)"""
    return _verify_dev("blsmi_kzg_verify_batch_jac_dev", d_srs_g1_jac, d_srs_g2_jac, d_commitments_jac, d_proofs_jac, d_z, d_y, m, d_ok, scalars, block, stream)


def _verify_blob(name, jac, srs_g1, srs_g2, polys, log2n, order, commitments, proofs, z, scalars, block, noncanon):
    pb, qb = (144, 288) if jac else (96, 192)
    log2n, order = _fr._shape(log2n, order)
    g, h = _e._u8(srs_g1, pb), _e._u8(srs_g2, 2 * qb)
    c, p = _e._u8(commitments), _e._u8(proofs)
    if c.size % pb or p.size != c.size:
        raise ValueError("expected m*%d bytes of C_j and as many of pi_j, got %d and %d" % (pb, c.size, p.size))
    m = c.size // pb
    zz, pp = _e._u8(z, 32 * m), _e._u8(polys, (32 << log2n) * m)
    pr = _e._scalars(scalars, m)
    block = _e._block(block)
    ok = np.zeros(max(1, m), dtype=np.uint8)
    nc = np.zeros(max(1, m), dtype=np.uint8) if noncanon else None
    comb, nre = C.c_int(0), C.c_size_t(0)
    g, h, c, p = (_e._recs(v, v.size, jac) for v in (g, h, c, p))
    _e._call(name, g, h, _e._p8(pp), log2n, order, c, p, _e._p8(zz), m, pr, block, _e._p8(ok), _e._p8(nc), C.byref(comb), C.byref(nre))
    return ok[:m].copy(), (nc[:m].astype(bool) if noncanon else None), comb.value, nre.value


def verify_blob_batch(srs_g1, srs_g2, polys, log2n, commitments, proofs, z, order=1, scalars=None, block=0, noncanon=True):
    """blsmi_kzg_verify_blob_batch -> (ok (m,) uint8, noncanon (m,) bool or None, combined, rechecked): m KZG blob proofs under one key.
    polys: m polynomials of N = 2^log2n values each (32 big-endian bytes, any value taken mod r) over the N-th roots of unity -- order 1:
    bit-reversed, the blob layout; order 0: position i holds w^i --; the rest as verify_batch, whose verdict on (C_j, pi_j, z_j, p_j(z_j))
    ok[j] is.  noncanon[j]: one of blob j's values was >= r, for the caller to reject (noncanon=False: not asked for).  z is an input:
    deriving it by Fiat-Shamir stays the caller's here; verify_blob_batch_wire derives it on the device."""
    return _verify_blob("blsmi_kzg_verify_blob_batch", False, srs_g1, srs_g2, polys, log2n, order, commitments, proofs, z, scalars, block, noncanon)


def verify_blob_batch_jac(srs_g1_jac, srs_g2_jac, polys, log2n, commitments_jac, proofs_jac, z, order=1, scalars=None, block=0, noncanon=True):
    """the same over in-memory points (144 / 288 bytes each, z == 0: infinity)"""
    return _verify_blob("blsmi_kzg_verify_blob_batch_jac", True, srs_g1_jac, srs_g2_jac, polys, log2n, order, commitments_jac, proofs_jac, z, scalars, block, noncanon)


def _verify_blob_dev(name, d_srs_g1, d_srs_g2, d_polys, log2n, order, d_commitments, d_proofs, d_z, m, d_ok, d_noncanon, scalars, block, stream):
    log2n, order = _fr._shape(log2n, order)
    pr = _e._scalars(scalars, m)
    comb, nre = C.c_int(0), C.c_size_t(0)
    _e._call(name, d_srs_g1, d_srs_g2, d_polys, log2n, order, d_commitments, d_proofs, d_z, m, pr, _e._block(block), d_ok, d_noncanon, C.byref(comb), C.byref(nre), stream)
    return comb.value, nre.value


def verify_blob_batch_dev(d_srs_g1, d_srs_g2, d_polys, log2n, order, d_commitments, d_proofs, d_z, m, d_ok, d_noncanon=0, scalars=None, block=0, stream=0):
    """device-pointer form (ints) over affine records; the m verdict bytes are in d_ok (and the m flags in d_noncanon, unless 0) when the
    call returns; scalars stay on the host.  -> (combined, rechecked)"""
    return _verify_blob_dev("blsmi_kzg_verify_blob_batch_dev", d_srs_g1, d_srs_g2, d_polys, log2n, order, d_commitments, d_proofs, d_z, m, d_ok, d_noncanon, scalars, block, stream)


def verify_blob_batch_jac_dev(d_srs_g1_jac, d_srs_g2_jac, d_polys, log2n, order, d_commitments_jac, d_proofs_jac, d_z, m, d_ok, d_noncanon=0, scalars=None, block=0, stream=0):
    """device-pointer form over in-memory points -> (combined, rechecked)"""
    return _verify_blob_dev("blsmi_kzg_verify_blob_batch_jac_dev", d_srs_g1_jac, d_srs_g2_jac, d_polys, log2n, order, d_commitments_jac, d_proofs_jac, d_z, m, d_ok, d_noncanon, scalars, block, stream)


def blob_challenge_batch(polys, log2n, commitments48):
    """blsmi_kzg_blob_challenge_batch -> z (m, 32) uint8: z[j] = SHA-256("FSBLOBVERIFY_V1_" || N as 16 big-endian bytes || blob_j ||
    commitment_j) mod r, EIP-4844's compute_challenge.  polys: m blobs of N = 2^log2n values of 32 bytes; commitments48: m compressed
    commitments.  The bytes are hashed as they are: nothing is decoded or validated."""
    log2n, _ = _fr._shape(log2n, 1)
    c = _e._u8(commitments48)
    if c.size % 48:
        raise ValueError("expected m*48 bytes of compressed commitments, got %d" % c.size)
    m = c.size // 48
    pp = _e._u8(polys, (32 << log2n) * m)
    z = np.zeros((m, 32), dtype=np.uint8)
    _e._call("blsmi_kzg_blob_challenge_batch", _e._p8(pp), log2n, _e._p8(c), _e._p8(z.reshape(-1)), m)
    return z


def blob_challenge_batch_dev(d_polys, log2n, d_commitments48, d_z, m, stream=0):
    """device-pointer form (ints); the m challenges are in d_z when the call returns"""
    log2n, _ = _fr._shape(log2n, 1)
    _e._call("blsmi_kzg_blob_challenge_batch_dev", d_polys, log2n, d_commitments48, d_z, m, stream)


def verify_blob_batch_wire(srs_g1, srs_g2, polys, log2n, commitments48, proofs48, scalars=None, block=0, status=True):
    """blsmi_kzg_verify_blob_batch_wire -> (ok (m,) uint8, status (m,) uint8 or None, combined, rechecked): EIP-4844's
    verify_blob_kzg_proof_batch from the bytes its caller holds.  polys: m blobs of N = 2^log2n values (32 big-endian bytes, the blob's
    own order); commitments48, proofs48: m compressed points each; the key, scalars and block as verify_blob_batch.  status[j] = errC |
    errPi << 3 | noncanon << 6 (the error codes of engine.g1_decompress_batch); ok[j] = 1 exactly when status[j] == 0 and verify_batch's
    verdict on (C_j, pi_j, z_j, p_j(z_j)) is 1, z_j being blob_challenge_batch's.  status=False: not asked for."""
    log2n, _ = _fr._shape(log2n, 1)
    g, h = _e._u8(srs_g1, 96), _e._u8(srs_g2, 2 * 192)
    c, p = _e._u8(commitments48), _e._u8(proofs48)
    if c.size % 48 or p.size != c.size:
        raise ValueError("expected m*48 bytes of C_j and as many of pi_j, got %d and %d" % (c.size, p.size))
    m = c.size // 48
    pp = _e._u8(polys, (32 << log2n) * m)
    pr = _e._scalars(scalars, m)
    block = _e._block(block)
    ok = np.zeros(max(1, m), dtype=np.uint8)
    st = np.zeros(max(1, m), dtype=np.uint8) if status else None
    comb, nre = C.c_int(0), C.c_size_t(0)
    _e._call("blsmi_kzg_verify_blob_batch_wire", _e._p8(g), _e._p8(h), _e._p8(pp), log2n, _e._p8(c), _e._p8(p), m, pr, block, _e._p8(ok), _e._p8(st),
             C.byref(comb), C.byref(nre))
    return ok[:m].copy(), (st[:m].copy() if status else None), comb.value, nre.value


def verify_blob_batch_wire_dev(d_srs_g1, d_srs_g2, d_polys, log2n, d_commitments48, d_proofs48, m, d_ok, d_status=0, scalars=None, block=0, stream=0):
    """device-pointer form (ints) over the key's affine records; the m verdict bytes are in d_ok (and the m status bytes in d_status, unless
    0) when the call returns; scalars stay on the host.  -> (combined, rechecked)"""
    log2n, _ = _fr._shape(log2n, 1)
    pr = _e._scalars(scalars, m)
    comb, nre = C.c_int(0), C.c_size_t(0)
    _e._call("blsmi_kzg_verify_blob_batch_wire_dev", d_srs_g1, d_srs_g2, d_polys, log2n, d_commitments48, d_proofs48, m, pr, _e._block(block), d_ok, d_status,
             C.byref(comb), C.byref(nre), stream)
    return comb.value, nre.value


_R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


def cell_shifts(log2_cells, log2n):
    """the shifts of the 2^log2_cells cells of 2^log2n values each that make up an EIP-7594 extended blob, as (cells, 32) uint8: cell k is the
    coset h_k <w_n> in bit-reversed order (order = 1) with h_k = w_N^bitrev(k), N = cells * n, k's log2_cells bits reversed -- position i of
    cell k is roots_of_unity_brp[n k + i].  Pure Python, big integers."""
    log2_cells, log2n = int(log2_cells), int(log2n)
    if log2_cells < 0 or log2n < 0 or log2_cells + log2n > 32:
        raise ValueError("log2_cells + log2n is 0 .. 32, got %d + %d" % (log2_cells, log2n))
    w = pow(7, (_R - 1) >> (log2_cells + log2n), _R)
    out = np.zeros((1 << log2_cells, 32), dtype=np.uint8)
    for k in range(1 << log2_cells):
        rev = int(format(k, "0%db" % log2_cells)[::-1], 2) if log2_cells else 0
        out[k] = np.frombuffer(pow(w, rev, _R).to_bytes(32, "big"), dtype=np.uint8)
    return out


def _verify_cell(name, jac, srs_g1, srs_g2, vals, log2n, order, shifts, commitments, proofs, scalars, block, flags):
    pb, qb = (144, 288) if jac else (96, 192)
    log2n, order = _fr._interp_shape(log2n, order)
    g, h = _e._u8(srs_g1, pb << log2n), _e._u8(srs_g2, 2 * qb)
    c, p = _e._u8(commitments), _e._u8(proofs)
    if c.size % pb or p.size != c.size:
        raise ValueError("expected m*%d bytes of C_j and as many of pi_j, got %d and %d" % (pb, c.size, p.size))
    m = c.size // pb
    hh, vv = _e._u8(shifts, 32 * m), _e._u8(vals, (32 << log2n) * m)
    pr = _e._scalars(scalars, m)
    block = _e._block(block)
    ok = np.zeros(max(1, m), dtype=np.uint8)
    fl = np.zeros(max(1, m), dtype=np.uint8) if flags else None
    comb, nre = C.c_int(0), C.c_size_t(0)
    g, h, c, p = (_e._recs(v, v.size, jac) for v in (g, h, c, p))
    _e._call(name, g, h, _e._p8(vv), log2n, order, _e._p8(hh), c, p, m, pr, block, _e._p8(ok), _e._p8(fl), C.byref(comb), C.byref(nre))
    return ok[:m].copy(), (fl[:m].copy() if flags else None), comb.value, nre.value


def verify_cell_batch(srs_g1, srs_g2, vals, log2n, shifts, commitments, proofs, order=1, scalars=None, block=0, flags=True):
    """blsmi_kzg_verify_cell_batch -> (ok (m,) uint8, flags (m,) uint8 or None, combined, rechecked): m KZG cell proofs under one key.
    srs_g1: [tau^0] G .. [tau^(n-1)] G, n = 2^log2n; srs_g2: H, [tau^n] H; vals: m cells of n values each (32 big-endian bytes, any value
    taken mod r) over the cosets shifts[j] <w> -- order 1: bit-reversed, a cell as it arrives; order 0: position i is the value at h w^i --;
    the rest as verify_batch.  flags[j]: bit 0 a value or the shift was >= r, bit 1 the shift is 0 mod r, for the caller to reject
    (flags=False: not asked for)."""
    return _verify_cell("blsmi_kzg_verify_cell_batch", False, srs_g1, srs_g2, vals, log2n, order, shifts, commitments, proofs, scalars, block, flags)


def verify_cell_batch_jac(srs_g1_jac, srs_g2_jac, vals, log2n, shifts, commitments_jac, proofs_jac, order=1, scalars=None, block=0, flags=True):
    """the same over in-memory points (144 / 288 bytes each, z == 0: infinity)"""
    return _verify_cell("blsmi_kzg_verify_cell_batch_jac", True, srs_g1_jac, srs_g2_jac, vals, log2n, order, shifts, commitments_jac, proofs_jac, scalars, block, flags)


def _verify_cell_dev(name, d_srs_g1, d_srs_g2, d_vals, log2n, order, d_shifts, d_commitments, d_proofs, m, d_ok, d_flags, scalars, block, stream):
    log2n, order = _fr._interp_shape(log2n, order)
    pr = _e._scalars(scalars, m)
    comb, nre = C.c_int(0), C.c_size_t(0)
    _e._call(name, d_srs_g1, d_srs_g2, d_vals, log2n, order, d_shifts, d_commitments, d_proofs, m, pr, _e._block(block), d_ok, d_flags, C.byref(comb), C.byref(nre), stream)
    return comb.value, nre.value


def verify_cell_batch_dev(d_srs_g1, d_srs_g2, d_vals, log2n, order, d_shifts, d_commitments, d_proofs, m, d_ok, d_flags=0, scalars=None, block=0, stream=0):
    """device-pointer form (ints) over affine records; the m verdict bytes are in d_ok (and the m flags in d_flags, unless 0) when the call
    returns; scalars stay on the host.  -> (combined, rechecked)"""
    return _verify_cell_dev("blsmi_kzg_verify_cell_batch_dev", d_srs_g1, d_srs_g2, d_vals, log2n, order, d_shifts, d_commitments, d_proofs, m, d_ok, d_flags, scalars, block, stream)


def verify_cell_batch_jac_dev(d_srs_g1_jac, d_srs_g2_jac, d_vals, log2n, order, d_shifts, d_commitments_jac, d_proofs_jac, m, d_ok, d_flags=0, scalars=None, block=0, stream=0):
    """device-pointer form over in-memory points -> (combined, rechecked)"""
    return _verify_cell_dev("blsmi_kzg_verify_cell_batch_jac_dev", d_srs_g1_jac, d_srs_g2_jac, d_vals, log2n, order, d_shifts, d_commitments_jac, d_proofs_jac, m, d_ok, d_flags, scalars, block, stream)
