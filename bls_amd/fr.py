"""The scalar field Fr on the device (blsmi 0.21): blsmi_fr_mul_batch[_dev], blsmi_fr_inv_batch[_dev] and the evaluation of polynomials in
evaluation form, blsmi_fr_eval_batch[_dev], over the same binder as bls_amd.engine (engine._fn / engine._call: the types come from
include/blsmi.h).  Host code only: every computation happens in the HIP kernels; a missing library or device raises, nothing falls back."""
import numpy as np

from . import engine as _e

MAX_LOG2N = 16


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
