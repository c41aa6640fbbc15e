"""The scalar field Fr on the device (blsmi 0.21): blsmi_fr_mul_batch[_dev], blsmi_fr_inv_batch[_dev] and the evaluation of polynomials in
evaluation form, blsmi_fr_eval_batch[_dev], and the interpolation over a coset (blsmi 0.22: blsmi_fr_coset_interp_batch[_dev]), over the same binder as bls_amd.engine (engine._fn / engine._call: the types come from
include/blsmi.h).  Host code only: every computation happens in the HIP kernels; a missing library or device raises, nothing falls back."""
import numpy as np

from . import engine as _e

MAX_LOG2N = 16
MAX_INTERP_LOG2N = 10


def _count(a, what):
    if a.size % 32:
        raise ValueError("%s: expected n*32 bytes, got %d" % (what, a.size))
    return a.size // 32


def mul_batch(a, b):
    """blsmi_fr_mul_batch -> (n, 32) uint8: a[t] b[t] mod r.  a, b: n scalars of 32 big-endian bytes each, any 256-bit value taken mod r"""
    pa, pb = _e._u8(a), _e._u8(b)
    n = _count(pa, "a")
    if pb.size != pa.size:
        raise ValueError("expected as many bytes of b as of a (%d), got %d" % (pa.size, pb.size))
    out = np.zeros((n, 32), dtype=np.uint8)
    _e._call("blsmi_fr_mul_batch", _e._p8(pa), _e._p8(pb), _e._p8(out.reshape(-1)), n)
    return out


def mul_batch_dev(d_a, d_b, d_out, n, stream=0):
    """device-pointer form (ints); the n products are in d_out when the call returns"""
    _e._call("blsmi_fr_mul_batch_dev", d_a, d_b, d_out, n, stream)


def inv_batch(a):
    """blsmi_fr_inv_batch -> (n, 32) uint8: the inverse of a[t] mod r, and 0 for 0 mod r"""
    pa = _e._u8(a)
    n = _count(pa, "a")
    out = np.zeros((n, 32), dtype=np.uint8)
    _e._call("blsmi_fr_inv_batch", _e._p8(pa), _e._p8(out.reshape(-1)), n)
    return out


def inv_batch_dev(d_a, d_out, n, stream=0):
    """device-pointer form (ints); the n inverses are in d_out when the call returns"""
    _e._call("blsmi_fr_inv_batch_dev", d_a, d_out, n, stream)


def _shape(log2n, order):
    log2n, order = int(log2n), int(order)
    if not 0 <= log2n <= MAX_LOG2N:
        raise ValueError("log2n is 0 .. %d, got %d" % (MAX_LOG2N, log2n))
    if order not in (0, 1):
        raise ValueError("order is 0 (position i holds w^i) or 1 (bit-reversed, the blob layout), got %d" % order)
    return log2n, order


def eval_batch(polys, log2n, z, order=0, noncanon=True):
    """blsmi_fr_eval_batch -> (y (m, 32) uint8, noncanon (m,) bool or None): y[j] = p_j(z_j) for m polynomials given by their N = 2^log2n
    values over the N-th roots of unity (32 big-endian bytes each, any value taken mod r); order as the header says; noncanon[j]: one of
    polynomial j's values was >= r (noncanon=False: not asked for, NULL goes to the library)"""
    log2n, order = _shape(log2n, order)
    zz = _e._u8(z)
    m = _count(zz, "z")
    pp = _e._u8(polys, (32 << log2n) * m)
    y = np.zeros((m, 32), dtype=np.uint8)
    nc = np.zeros(m, dtype=np.uint8) if noncanon else None
    _e._call("blsmi_fr_eval_batch", _e._p8(pp), log2n, order, _e._p8(zz), _e._p8(y.reshape(-1)), _e._p8(nc), m)
    return y, (nc.astype(bool) if noncanon else None)


def eval_batch_dev(d_polys, log2n, order, d_z, d_y, d_noncanon, m, stream=0):
    """device-pointer form (ints; d_noncanon 0: not asked for); the m values are in d_y when the call returns"""
    log2n, order = _shape(log2n, order)
    _e._call("blsmi_fr_eval_batch_dev", d_polys, log2n, order, d_z, d_y, d_noncanon, m, stream)


def _interp_shape(log2n, order):
    log2n, order = int(log2n), int(order)
    if not 0 <= log2n <= MAX_INTERP_LOG2N:
        raise ValueError("log2n is 0 .. %d, got %d" % (MAX_INTERP_LOG2N, log2n))
    if order not in (0, 1):
        raise ValueError("order is 0 (position i is the value at h w^i) or 1 (bit-reversed, a cell as it arrives), got %d" % order)
    return log2n, order


def coset_interp_batch(vals, log2n, shifts, order=0, shift_pow=True, flags=True):
    """blsmi_fr_coset_interp_batch -> (coeffs (m, n, 32) uint8, shift_pow (m, 32) uint8 or None, flags (m,) uint8 or None): the n = 2^log2n
    coefficients (natural order, fully reduced) of the polynomial below degree n with the values vals[j] over the coset shifts[j] <w>, 32
    big-endian bytes each, any value taken mod r; order as the header says; shift_pow[j] = h_j^n mod r; flags[j]: bit 0 a value or the shift
    was >= r, bit 1 the shift is 0 mod r (shift_pow=False / flags=False: not asked for, NULL goes to the library)"""
    log2n, order = _interp_shape(log2n, order)
    hh = _e._u8(shifts)
    m = _count(hh, "shifts")
    vv = _e._u8(vals, (32 << log2n) * m)
    co = np.zeros((m, 1 << log2n, 32), dtype=np.uint8)
    sp = np.zeros((m, 32), dtype=np.uint8) if shift_pow else None
    fl = np.zeros(m, dtype=np.uint8) if flags else None
    _e._call("blsmi_fr_coset_interp_batch", _e._p8(vv), log2n, order, _e._p8(hh), _e._p8(co.reshape(-1)), _e._p8(sp.reshape(-1)) if shift_pow else None, _e._p8(fl), m)
    return co, sp, fl


def coset_interp_batch_dev(d_vals, log2n, order, d_shifts, d_coeffs, d_shift_pow, d_flags, m, stream=0):
    """device-pointer form (ints; d_shift_pow / d_flags 0: not asked for); the m * n coefficients are in d_coeffs when the call returns"""
    log2n, order = _interp_shape(log2n, order)
    _e._call("blsmi_fr_coset_interp_batch_dev", d_vals, log2n, order, d_shifts, d_coeffs, d_shift_pow, d_flags, m, stream)
