"""Thin ctypes layer over the C ABI of libblsmi.so (include/blsmi.h).  Host code only: every
computation happens in the HIP kernels; a missing library or device raises, nothing falls back."""
import ctypes as C

import numpy as np

from . import _native

_u8p = C.POINTER(C.c_uint8)
_u64p = C.POINTER(C.c_uint64)


class BlsmiError(RuntimeError):
    pass


_ERR = {-1: "no usable HIP device", -2: "HIP runtime call failed", -3: "bad argument", -4: "out of memory", -5: "RCCL unavailable or collective failed", -6: "OS random source failed"}


def _check(rc, what):
    if rc != 0:
        raise BlsmiError("%s failed: %s (%d)" % (what, _ERR.get(rc, "unknown"), rc))


def _lib():
    return _native.load()


def _u8(x, nbytes=None):
    a = np.frombuffer(x, dtype=np.uint8) if isinstance(x, (bytes, bytearray, memoryview)) else np.ascontiguousarray(x, dtype=np.uint8).reshape(-1)
    if nbytes is not None and a.size != nbytes:
        raise ValueError("expected %d bytes, got %d" % (nbytes, a.size))
    return a


def _p8(a):
    return a.ctypes.data_as(_u8p) if a is not None and a.size else None


def init(device=0):
    """Bind this process to one device (one rank per GPU under torchrun)."""
    _check(_lib().blsmi_init(int(device)), "blsmi_init")


def init_devices(ndev=0):
    """Drive the first ndev devices (0 = all visible) from this one process: large verify / pairing batches are split
    over them inside the library (RCCL bitmap all-reduce / partial-product all-gather), see include/blsmi.h."""
    _check(_lib().blsmi_init_devices(int(ndev)), "blsmi_init_devices")


def debug_alias_own(ptr, nbytes, device_index):
    """TEST HOOK (BLSMI_DEVICE_ALIAS): the device-pointer range belongs to logical device `device_index` (include/blsmi.h)."""
    _check(_lib().blsmi_debug_alias_own(C.c_void_p(int(ptr)), C.c_size_t(int(nbytes)), int(device_index)), "blsmi_debug_alias_own")


def trim(keep_bytes_per_context=0):
    """Give the temporaries idle call contexts hold beyond keep_bytes_per_context (and the pool cache) back to the driver; bytes freed."""
    freed = C.c_size_t(0)
    _check(_lib().blsmi_trim(C.c_size_t(int(keep_bytes_per_context)), C.byref(freed)), "blsmi_trim")
    return int(freed.value)


def held_bytes():
    """device memory the call contexts currently hold for temporaries (all devices)"""
    _lib().blsmi_held_bytes.restype = C.c_size_t
    return int(_lib().blsmi_held_bytes())


SHAPE_PAIRING, SHAPE_MILLER_LOOP, SHAPE_FINAL_EXP, SHAPE_G2_PREPARE, SHAPE_VERIFY, SHAPE_SIGN, SHAPE_VERIFY_DOMAIN, SHAPE_POINT_ADD = range(8)


def prefer_cpu(shape, n):
    """True when n operations of `shape` in one call finish sooner on one core of the upstream CPU path (include/blsmi.h)"""
    return bool(_lib().blsmi_prefer_cpu(int(shape), C.c_size_t(int(n))))


def device_leases(device_index):
    """context leases device `device_index` has served since initialisation (-1: no such device)"""
    _lib().blsmi_debug_device_leases.restype = C.c_longlong
    return int(_lib().blsmi_debug_device_leases(int(device_index)))


def device_count():
    return int(_lib().blsmi_device_count())


def shard_count():
    return int(_lib().blsmi_shard_count())


def set_latency_threshold(max_tuples):
    """Batches of at most max_tuples tuples take the latency path (one tuple per wave); 0 = always the lane-pair kernels."""
    _check(_lib().blsmi_set_latency_threshold(C.c_size_t(int(max_tuples))), "blsmi_set_latency_threshold")


def set_quad_threshold(max_tuples):
    """Batches above the latency threshold and of at most max_tuples tuples take the lane-quad kernels (four lanes per tuple); 0 = off."""
    _check(_lib().blsmi_set_quad_threshold(C.c_size_t(int(max_tuples))), "blsmi_set_quad_threshold")


def set_row_threshold(min_tuples, max_tuples):
    """A lone pairing / verify call of min_tuples .. max_tuples tuples takes the lane-row kernels (sixteen lanes per tuple); max 0 = off."""
    _check(_lib().blsmi_set_row_threshold(C.c_size_t(int(min_tuples)), C.c_size_t(int(max_tuples))), "blsmi_set_row_threshold")


ROW_DEFAULT = (2048, 8192)


def set_option(name, value):
    """run-time switch between code paths with identical results: "agg_cofactor_pow", "msm_sort", "dup_force_sort" (include/blsmi.h)"""
    _check(_lib().blsmi_set_option(name.encode(), C.c_longlong(int(value))), "blsmi_set_option(%s)" % name)


def set_mul_assume_subgroup(on=True):
    """scalar multiplications through the curve endomorphisms (multiplicands in the prime-order subgroup; the default) or,
    with on=False, the plain windowed ladder that serves every curve point"""
    _check(_lib().blsmi_set_mul_assume_subgroup(C.c_int(1 if on else 0)), "blsmi_set_mul_assume_subgroup")


def shutdown():
    _lib().blsmi_shutdown.restype = None
    _lib().blsmi_shutdown()


def version():
    return _lib().blsmi_version().decode()


class PackedMsgs:
    """n messages already laid out as the C ABI wants them (concatenated bytes + n+1 offsets): lets a caller that issues
    the same batch repeatedly -- or holds a million messages -- pay the Python-side packing once."""

    def __init__(self, msgs):
        self.buf, self.off = _msgs(msgs)
        self.n = len(msgs)

    def __len__(self):
        return self.n


def _msgs(msgs):
    if isinstance(msgs, PackedMsgs):
        return msgs.buf, msgs.off
    off = np.zeros(len(msgs) + 1, dtype=np.uint64)
    if len(msgs):
        off[1:] = np.cumsum([len(m) for m in msgs])
    buf = np.frombuffer(b"".join(bytes(m) for m in msgs) or b"\0", dtype=np.uint8)
    return buf, off


# ---- pairing ---------------------------------------------------------------------------------------
class HostBuffer:
    """Page-locked host memory from the library (blsmi_host_alloc) as a numpy uint8 array: `.a`.  Arrays handed to the host entry
    points from such memory are copied by DMA instead of being staged.  The block is returned to the runtime when the LAST numpy view of
    it is gone: `.a` and every slice taken from it keep the allocation alive (they hold the ctypes block whose finaliser frees it), so
    .free() -- or dropping the HostBuffer -- can never pull memory from under a view that is still in use."""

    def __init__(self, nbytes):
        import weakref
        p = C.c_void_p()
        lib = _lib()
        lib.blsmi_host_alloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
        lib.blsmi_host_free.argtypes = [C.c_void_p]
        _check(lib.blsmi_host_alloc(C.c_size_t(int(nbytes)), C.byref(p)), "blsmi_host_alloc")
        self.nbytes = int(nbytes)
        if nbytes:
            block = (C.c_uint8 * self.nbytes).from_address(p.value)         # every numpy view below references this object
            self._finalizer = weakref.finalize(block, lib.blsmi_host_free, C.c_void_p(p.value))
            self.a = np.frombuffer(block, dtype=np.uint8)
        else:
            self._finalizer = None
            self.a = np.zeros(0, np.uint8)

    @property
    def alive(self):
        """False once the block has gone back to the runtime (no view of it is left)"""
        return self._finalizer is not None and self._finalizer.alive

    def free(self):
        """drop this object's reference; the memory is released as soon as no view of `.a` remains (at once if there is none)"""
        self.a = None


def pairing_batch(g1_aff, g2_aff, n, out=None):
    """n x 96 B G1 affine, n x 192 B G2 affine -> (n, 72) uint64: the reference's in-memory FQ12."""
    a, b = _u8(g1_aff, 96 * n), _u8(g2_aff, 192 * n)
    if out is None:
        out = np.zeros((n, 72), dtype=np.uint64)
    _check(_lib().blsmi_pairing_batch(_p8(a), _p8(b), out.ctypes.data_as(_u64p), C.c_size_t(n)), "blsmi_pairing_batch")
    return out


def miller_loop_batch(g1_aff, g2_aff, n):
    a, b = _u8(g1_aff, 96 * n), _u8(g2_aff, 192 * n)
    out = np.zeros((n, 72), dtype=np.uint64)
    _check(_lib().blsmi_miller_loop_batch(_p8(a), _p8(b), out.ctypes.data_as(_u64p), C.c_size_t(n)), "blsmi_miller_loop_batch")
    return out


def final_exponentiation_batch(fq12):
    x = np.ascontiguousarray(fq12, dtype=np.uint64).reshape(-1, 72)
    out = np.zeros_like(x)
    _check(_lib().blsmi_final_exponentiation_batch(x.ctypes.data_as(_u64p), out.ctypes.data_as(_u64p), C.c_size_t(x.shape[0])), "blsmi_final_exponentiation_batch")
    return out


def pairing_batch_dev(d_g1, d_g2, d_out, n, stream=0):
    """Device-pointer form (ints, e.g. torch.Tensor.data_ptr()); enqueues and synchronises `stream`."""
    _check(_lib().blsmi_pairing_batch_dev(C.c_void_p(d_g1), C.c_void_p(d_g2), C.c_void_p(d_out), C.c_size_t(n), C.c_void_p(stream)), "blsmi_pairing_batch_dev")


def verify_batch_dev(group, d_msgs, d_off, d_pks, d_sigs, d_inf, d_ok, n, stream=0):
    fn = _lib().blsmi_g2pubs_verify_batch_dev if group == "g2pubs" else _lib().blsmi_g1pubs_verify_batch_dev
    _check(fn(C.c_void_p(d_msgs), C.c_void_p(d_off), C.c_void_p(d_pks), C.c_void_p(d_sigs), C.c_void_p(d_inf or 0), C.c_void_p(d_ok), C.c_size_t(n), C.c_void_p(stream)), "verify_batch_dev")


def g1pubs_verify_with_domain_batch_dev(d_msgs32, d_domain, d_pks, d_sigs, d_inf, d_ok, n, stream=0):
    """VerifyWithDomain (g1pubs/bls.go:171-174) with everything resident on the device (ints = device pointers)"""
    _check(_lib().blsmi_g1pubs_verify_with_domain_batch_dev(C.c_void_p(d_msgs32), C.c_void_p(d_domain), C.c_void_p(d_pks), C.c_void_p(d_sigs), C.c_void_p(d_inf or 0), C.c_void_p(d_ok), C.c_size_t(n), C.c_void_p(stream)), "verify_with_domain_batch_dev")


def mul_batch_dev(group, d_pts, d_scalars, d_out, d_out_inf, n, stream=0, any_point=False):
    """k_i * P_i with everything resident on the device (ints = device pointers; d_pts = 0: the group generator).
    any_point: multiplicands outside the prime-order subgroup are allowed for this call (see g1_mul_batch)."""
    if any_point:
        fn = _lib().blsmi_g1_mul_batch_dev_ex if group == "g1" else _lib().blsmi_g2_mul_batch_dev_ex
        _check(fn(C.c_void_p(d_pts or 0), C.c_void_p(d_scalars), C.c_void_p(d_out), C.c_void_p(d_out_inf), C.c_size_t(n), C.c_void_p(stream), C.c_uint(MUL_ANY_POINT)), "mul_batch_dev_ex")
        return
    fn = _lib().blsmi_g1_mul_batch_dev if group == "g1" else _lib().blsmi_g2_mul_batch_dev
    _check(fn(C.c_void_p(d_pts or 0), C.c_void_p(d_scalars), C.c_void_p(d_out), C.c_void_p(d_out_inf), C.c_size_t(n), C.c_void_p(stream)), "mul_batch_dev")


def sum_dev(group, d_pts, d_in_inf, n, d_out, stream=0):
    """sum of n resident points -> affine bytes at d_out (device); returns True when the sum is the point at infinity."""
    fn = _lib().blsmi_g1_sum_dev if group == "g1" else _lib().blsmi_g2_sum_dev
    oinf = C.c_int(0)
    _check(fn(C.c_void_p(d_pts), C.c_void_p(d_in_inf or 0), C.c_size_t(n), C.c_void_p(d_out), C.byref(oinf), C.c_void_p(stream)), "sum_dev")
    return bool(oinf.value)


def msm_dev(group, d_pts, d_scalars, n, d_out, stream=0, any_point=False):
    """sum_i k_i P_i over resident points and scalars -> affine bytes at d_out (device); True when it is the point at infinity."""
    oinf = C.c_int(0)
    if any_point:
        fn = _lib().blsmi_g1_msm_dev_ex if group == "g1" else _lib().blsmi_g2_msm_dev_ex
        _check(fn(C.c_void_p(d_pts), C.c_void_p(d_scalars), C.c_size_t(n), C.c_void_p(d_out), C.byref(oinf), C.c_void_p(stream), C.c_uint(MUL_ANY_POINT)), "msm_dev_ex")
        return bool(oinf.value)
    fn = _lib().blsmi_g1_msm_dev if group == "g1" else _lib().blsmi_g2_msm_dev
    _check(fn(C.c_void_p(d_pts), C.c_void_p(d_scalars), C.c_size_t(n), C.c_void_p(d_out), C.byref(oinf), C.c_void_p(stream)), "msm_dev")
    return bool(oinf.value)


def verify_aggregate_common_dev(group, d_pks, n, msg, sig, domain=None, stream=0):
    """VerifyAggregateCommon (g2pubs/bls.go:275-278, g1pubs/bls.go:287-297) with the n public keys resident on the device (int =
    device pointer); msg / sig = host bytes; domain (8 bytes, g1pubs only): the *WithDomain form over a 32-byte message."""
    ok = C.c_int(0)
    m = _u8(msg) if len(msg) else None
    if domain is not None:
        assert group == "g1pubs"
        _check(_lib().blsmi_g1pubs_verify_aggregate_common_with_domain_dev(C.c_void_p(d_pks or 0), C.c_size_t(n), _p8(_u8(msg, 32)), _p8(_u8(domain, 8)), _p8(_u8(sig, 192)), C.byref(ok), C.c_void_p(stream)), "verify_aggregate_common_with_domain_dev")
        return bool(ok.value)
    fn, sgb = (_lib().blsmi_g2pubs_verify_aggregate_common_dev, 96) if group == "g2pubs" else (_lib().blsmi_g1pubs_verify_aggregate_common_dev, 192)
    _check(fn(C.c_void_p(d_pks or 0), C.c_size_t(n), _p8(m) if m is not None else None, C.c_size_t(len(msg)), _p8(_u8(sig, sgb)), C.byref(ok), C.c_void_p(stream)), "verify_aggregate_common_dev")
    return bool(ok.value)


def verify_aggregate_dev(group, d_msgs, d_off, d_pks, sig, n, stream=0):
    """VerifyAggregate with messages / offsets / keys resident on the device; sig = host bytes of the aggregate signature."""
    fn, sgb = (_lib().blsmi_g2pubs_verify_aggregate_dev, 96) if group == "g2pubs" else (_lib().blsmi_g1pubs_verify_aggregate_dev, 192)
    s = _u8(sig, sgb)
    ok = C.c_int(0)
    _check(fn(C.c_void_p(d_msgs), C.c_void_p(d_off), C.c_void_p(d_pks), _p8(s), C.c_size_t(n), C.byref(ok), C.c_void_p(stream)), "verify_aggregate_dev")
    return bool(ok.value)


def verify_aggregate_with_domain_dev(d_msgs32, d_domain, d_pks, sig, n, stream=0):
    s = _u8(sig, 192)
    ok = C.c_int(0)
    _check(_lib().blsmi_g1pubs_verify_aggregate_with_domain_dev(C.c_void_p(d_msgs32), C.c_void_p(d_domain), C.c_void_p(d_pks), _p8(s), C.c_size_t(n), C.byref(ok), C.c_void_p(stream)), "verify_aggregate_with_domain_dev")
    return bool(ok.value)


# ---- prepared public keys (g2pubs): G2AffineToPrepared once, Miller loops that read the lines (blsmi 0.4) ----
G2_PREPARED_BYTES = 24704


def g2_prepare_batch_dev(d_g2_aff, n, d_prepared, stream=0):
    """n resident G2 points -> n tables of G2_PREPARED_BYTES at d_prepared (device)."""
    _check(_lib().blsmi_g2_prepare_batch_dev(C.c_void_p(d_g2_aff), C.c_size_t(n), C.c_void_p(d_prepared), C.c_void_p(stream)), "blsmi_g2_prepare_batch_dev")


def g2_prepared_export_dev(d_prepared, n, d_out, stream=0):
    """the reference's G2Prepared.coeffs of n tables: n x 68 x 3 x 12 uint64 at d_out (device)."""
    _check(_lib().blsmi_g2_prepared_export_dev(C.c_void_p(d_prepared), C.c_size_t(n), C.c_void_p(d_out), C.c_void_p(stream)), "blsmi_g2_prepared_export_dev")


def g2_prepare_batch(g2_aff, n):
    """G2AffineToPrepared (g2.go:639-801) of n host points: (n, 68, 3, 12) uint64 -- coefficient triples of FQ2 as c0 | c1 limbs."""
    q = _u8(g2_aff, 192 * n)
    out = np.empty((n, 68, 3, 12), dtype=np.uint64)
    _check(_lib().blsmi_g2_prepare_batch(_p8(q), C.c_size_t(n), out.ctypes.data_as(_u64p)), "blsmi_g2_prepare_batch")
    return out


class PreparedKeys:
    """n g2pubs public keys prepared into tables the library owns (blsmi_g2_prepared_create); .ptr is the device pointer."""

    def __init__(self, g2_aff, n):
        q = _u8(g2_aff, 192 * n)
        h = C.c_void_p(0)
        _check(_lib().blsmi_g2_prepared_create(_p8(q), C.c_size_t(n), C.byref(h)), "blsmi_g2_prepared_create")
        self.ptr, self.n = h.value, n

    def close(self):
        if self.ptr:
            _check(_lib().blsmi_g2_prepared_destroy(C.c_void_p(self.ptr)), "blsmi_g2_prepared_destroy")
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def g2pubs_verify_batch_prepared(msgs, prepared, key_idx, sigs, inf_flags=None):
    """g2pubs.Verify x n, host buffers, keys prepared (a PreparedKeys or a device pointer): (ok bool array, packed bitmap)."""
    n = len(msgs)
    buf, off = _msgs(msgs)
    ptr = prepared.ptr if isinstance(prepared, PreparedKeys) else prepared
    idx = None if key_idx is None else np.ascontiguousarray(key_idx, dtype=np.uint32)
    s = _u8(sigs, 96 * n)
    fl = None if inf_flags is None else _u8(inf_flags, n)
    ok = np.empty(n, dtype=np.uint8)
    bm = np.empty((n + 7) // 8, dtype=np.uint8)
    _check(_lib().blsmi_g2pubs_verify_batch_prepared(_p8(buf), off.ctypes.data_as(_u64p), C.c_void_p(ptr), None if idx is None else idx.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                    _p8(s), _p8(fl), _p8(ok), _p8(bm), C.c_size_t(n)), "blsmi_g2pubs_verify_batch_prepared")
    return ok.astype(bool), bm


def pairing_batch_prepared_dev(d_g1, d_prepared, d_key_idx, d_out, n, stream=0):
    _check(_lib().blsmi_pairing_batch_prepared_dev(C.c_void_p(d_g1), C.c_void_p(d_prepared), C.c_void_p(d_key_idx or 0), C.c_void_p(d_out), C.c_size_t(n), C.c_void_p(stream)), "blsmi_pairing_batch_prepared_dev")


def g2pubs_verify_batch_prepared_dev(d_msgs, d_off, d_prepared, d_key_idx, d_sigs, d_inf, d_ok, n, stream=0):
    _check(_lib().blsmi_g2pubs_verify_batch_prepared_dev(C.c_void_p(d_msgs), C.c_void_p(d_off), C.c_void_p(d_prepared), C.c_void_p(d_key_idx or 0), C.c_void_p(d_sigs),
                                                        C.c_void_p(d_inf or 0), C.c_void_p(d_ok), C.c_size_t(n), C.c_void_p(stream)), "blsmi_g2pubs_verify_batch_prepared_dev")


def g2pubs_verify_aggregate_prepared(msgs, prepared, key_idx, sig):
    """Signature.VerifyAggregate over prepared keys, host buffers (a PreparedKeys or a device pointer)."""
    n = len(msgs)
    buf, off = _msgs(msgs)
    ptr = prepared.ptr if isinstance(prepared, PreparedKeys) else prepared
    idx = None if key_idx is None else np.ascontiguousarray(key_idx, dtype=np.uint32)
    s = _u8(sig, 96)
    ok = C.c_int(0)
    _check(_lib().blsmi_g2pubs_verify_aggregate_prepared(_p8(buf), off.ctypes.data_as(_u64p), C.c_void_p(ptr), None if idx is None else idx.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                        _p8(s), C.c_size_t(n), C.byref(ok)), "blsmi_g2pubs_verify_aggregate_prepared")
    return bool(ok.value)


def g2pubs_verify_aggregate_prepared_dev(d_msgs, d_off, d_prepared, d_key_idx, sig, n, stream=0):
    s = _u8(sig, 96)
    ok = C.c_int(0)
    _check(_lib().blsmi_g2pubs_verify_aggregate_prepared_dev(C.c_void_p(d_msgs), C.c_void_p(d_off), C.c_void_p(d_prepared), C.c_void_p(d_key_idx or 0), _p8(s), C.c_size_t(n),
                                                            C.byref(ok), C.c_void_p(stream)), "blsmi_g2pubs_verify_aggregate_prepared_dev")
    return bool(ok.value)


# ---- groups ----------------------------------------------------------------------------------------
MUL_ANY_POINT = 1          # BLSMI_MUL_ANY_POINT (include/blsmi.h)


def _mul(fn, pb, pts, scalars, n, flags=None):
    p, s = _u8(pts, pb * n), _u8(scalars, 32 * n)
    out = np.empty(pb * n, dtype=np.uint8)              # every byte is written by the call
    inf = np.empty(n, dtype=np.uint8)
    extra = () if flags is None else (C.c_uint(flags),)
    _check(fn(_p8(p), _p8(s), _p8(out), _p8(inf), C.c_size_t(n), *extra), "mul_batch")
    return out.reshape(n, pb), inf.astype(bool)


def g1_mul_batch(pts, scalars, n, any_point=False):
    """k_i * P_i (G1Affine.MulFR, g1.go:80-90).  The default ladder runs through the curve endomorphism and REQUIRES multiplicands
    in the prime-order subgroup (hash points, generators, keys / signatures that passed Deserialize's subgroup check): an on-curve
    point outside it gives a different point, silently.  any_point=True selects, for this call only, the plain windowed ladder
    that serves every curve point like the reference does (e.g. after g1_decompress_batch(check_subgroup=False))."""
    if any_point:
        return _mul(_lib().blsmi_g1_mul_batch_ex, 96, pts, scalars, n, MUL_ANY_POINT)
    return _mul(_lib().blsmi_g1_mul_batch, 96, pts, scalars, n)


def g2_mul_batch(pts, scalars, n, any_point=False):
    """k_i * P_i (G2Affine.MulFR, g2.go:92-102); subgroup points unless any_point=True -- see g1_mul_batch."""
    if any_point:
        return _mul(_lib().blsmi_g2_mul_batch_ex, 192, pts, scalars, n, MUL_ANY_POINT)
    return _mul(_lib().blsmi_g2_mul_batch, 192, pts, scalars, n)


def _mul_gen(fn, pb, scalars, n):
    s = _u8(scalars, 32 * n)
    out = np.zeros(pb * n, dtype=np.uint8)
    inf = np.zeros(n, dtype=np.uint8)
    _check(fn(_p8(s), _p8(out), _p8(inf), C.c_size_t(n)), "mul_generator_batch")
    return out.reshape(n, pb), inf.astype(bool)


def g1_mul_generator_batch(scalars, n):
    """k_i * G1 generator (PrivToPub of g1pubs)."""
    return _mul_gen(_lib().blsmi_g1_mul_generator_batch, 96, scalars, n)


def g2_mul_generator_batch(scalars, n):
    """k_i * G2 generator (PrivToPub of g2pubs)."""
    return _mul_gen(_lib().blsmi_g2_mul_generator_batch, 192, scalars, n)


def _msm(fn, pb, pts, scalars, n, flags=None):
    p = _u8(pts, pb * n) if n else np.zeros(1, np.uint8)
    s = _u8(scalars, 32 * n) if n else np.zeros(1, np.uint8)
    out = np.zeros(pb, dtype=np.uint8)
    oinf = C.c_int(0)
    extra = () if flags is None else (C.c_uint(flags),)
    _check(fn(_p8(p), _p8(s), C.c_size_t(n), _p8(out), C.byref(oinf), *extra), "msm")
    return None if oinf.value else out.tobytes()


def g1_msm(pts, scalars, n, any_point=False):
    """sum_i k_i * P_i -> 96 affine bytes, or None for the point at infinity (subgroup points unless any_point=True, see g1_mul_batch)."""
    if any_point:
        return _msm(_lib().blsmi_g1_msm_ex, 96, pts, scalars, n, MUL_ANY_POINT)
    return _msm(_lib().blsmi_g1_msm, 96, pts, scalars, n)


def g2_msm(pts, scalars, n, any_point=False):
    if any_point:
        return _msm(_lib().blsmi_g2_msm_ex, 192, pts, scalars, n, MUL_ANY_POINT)
    return _msm(_lib().blsmi_g2_msm, 192, pts, scalars, n)


def _sum(fn, pb, pts, n, in_inf):
    p = _u8(pts, pb * n) if n else np.zeros(1, np.uint8)
    f = _u8(in_inf, n) if in_inf is not None else None
    out = np.zeros(pb, dtype=np.uint8)
    oinf = C.c_int(0)
    _check(fn(_p8(p), _p8(f), C.c_size_t(n), _p8(out), C.byref(oinf)), "sum")
    return (None if oinf.value else out.tobytes())


def g1_sum(pts, n, in_inf=None):
    """Sum of n affine points -> 96 bytes, or None for the point at infinity."""
    return _sum(_lib().blsmi_g1_sum, 96, pts, n, in_inf)


def g2_sum(pts, n, in_inf=None):
    return _sum(_lib().blsmi_g2_sum, 192, pts, n, in_inf)


# ---- hash to curve ---------------------------------------------------------------------------------
def hash_g1_batch(msgs):
    buf, off = _msgs(msgs)
    out = np.zeros((len(msgs), 96), dtype=np.uint8)
    _check(_lib().blsmi_hash_g1_batch(_p8(buf), off.ctypes.data_as(_u64p), _p8(out.reshape(-1)), C.c_size_t(len(msgs))), "blsmi_hash_g1_batch")
    return out


def hash_g2_batch(msgs):
    buf, off = _msgs(msgs)
    out = np.zeros((len(msgs), 192), dtype=np.uint8)
    _check(_lib().blsmi_hash_g2_batch(_p8(buf), off.ctypes.data_as(_u64p), _p8(out.reshape(-1)), C.c_size_t(len(msgs))), "blsmi_hash_g2_batch")
    return out


def hash_g2_with_domain_batch(msgs32, domain8):
    n = len(msgs32)
    buf = _u8(b"".join(bytes(m) for m in msgs32), 32 * n)
    d = _u8(domain8, 8)
    out = np.zeros((n, 192), dtype=np.uint8)
    _check(_lib().blsmi_hash_g2_with_domain_batch(_p8(buf), _p8(d), _p8(out.reshape(-1)), C.c_size_t(n)), "blsmi_hash_g2_with_domain_batch")
    return out


# ---- sign: sk_i * H(m_i) in one call (the hash points stay on the device) ---------------------------
def _sign(fn, name, ob, n, head, sks):
    k = _u8(sks, 32 * n)
    out = np.zeros((n, ob), dtype=np.uint8); inf = np.zeros(n, dtype=np.uint8)
    _check(fn(*head, _p8(k), _p8(out.reshape(-1)), _p8(inf), C.c_size_t(n)), name)
    return out, inf


def g2pubs_sign_batch(msgs, sks):
    """blsmi_g2pubs_sign_batch: n x 96-byte signatures sk_i * HashG1(m_i) (g2pubs/bls.go:132-135) and their infinity flags"""
    buf, off = _msgs(msgs)
    return _sign(_lib().blsmi_g2pubs_sign_batch, "blsmi_g2pubs_sign_batch", 96, len(msgs), (_p8(buf), off.ctypes.data_as(_u64p)), sks)


def g1pubs_sign_batch(msgs, sks):
    """blsmi_g1pubs_sign_batch: n x 192-byte signatures sk_i * HashG2(m_i) (g1pubs/bls.go:132-135)"""
    buf, off = _msgs(msgs)
    return _sign(_lib().blsmi_g1pubs_sign_batch, "blsmi_g1pubs_sign_batch", 192, len(msgs), (_p8(buf), off.ctypes.data_as(_u64p)), sks)


def g1pubs_sign_with_domain_batch(msgs32, domain8, sks):
    """blsmi_g1pubs_sign_with_domain_batch: sk_i * HashG2WithDomain(m_i, domain) (g1pubs/bls.go:138-141)"""
    n = len(msgs32)
    buf = _u8(b"".join(bytes(m) for m in msgs32), 32 * n)
    d = _u8(domain8, 8)
    return _sign(_lib().blsmi_g1pubs_sign_with_domain_batch, "blsmi_g1pubs_sign_with_domain_batch", 192, n, (_p8(buf), _p8(d)), sks)


# ---- verify ----------------------------------------------------------------------------------------
def _verify_batch(fn, pkb, sgb, msgs, pks, sigs, inf_flags):
    n = len(msgs)
    buf, off = _msgs(msgs)
    p, s = _u8(pks, pkb * n), _u8(sigs, sgb * n)
    f = _u8(inf_flags, n) if inf_flags is not None else None
    ok = np.zeros(n, dtype=np.uint8)
    bitmap = np.zeros((n + 7) // 8, dtype=np.uint8)
    _check(fn(_p8(buf), off.ctypes.data_as(_u64p), _p8(p), _p8(s), _p8(f), _p8(ok), _p8(bitmap), C.c_size_t(n)), "verify_batch")
    return ok.astype(bool), bitmap


def g2pubs_verify_batch(msgs, pks, sigs, inf_flags=None):
    return _verify_batch(_lib().blsmi_g2pubs_verify_batch, 192, 96, msgs, pks, sigs, inf_flags)


def g1pubs_verify_batch(msgs, pks, sigs, inf_flags=None):
    return _verify_batch(_lib().blsmi_g1pubs_verify_batch, 96, 192, msgs, pks, sigs, inf_flags)


# ---- randomised batch verification (blsmi 0.8): one pairing check per batch, per-tuple verdicts only when it fails ---------------
def _scalars(scalars, n):
    """caller scalars (n nonzero 64-bit integers) as a uint64 array, or None: the library draws fresh ones"""
    if scalars is None:
        return None, None
    r = np.ascontiguousarray(np.asarray([int(x) for x in scalars], dtype=np.uint64))
    if r.shape != (n,):
        raise ValueError("need one scalar per tuple")
    return r, r.ctypes.data_as(_u64p)


def _verify_batch_rlc(fn, pkb, sgb, msgs, pks, sigs, inf_flags, scalars):
    n = len(msgs)
    buf, off = _msgs(msgs)
    p, s = _u8(pks, pkb * n), _u8(sigs, sgb * n)
    f = _u8(inf_flags, n) if inf_flags is not None else None
    r, pr = _scalars(scalars, n)
    ok = np.zeros(n, dtype=np.uint8)
    bitmap = np.zeros((n + 7) // 8, dtype=np.uint8)
    comb = C.c_int(0)
    _check(fn(_p8(buf), off.ctypes.data_as(_u64p), _p8(p), _p8(s), _p8(f), pr, _p8(ok), _p8(bitmap), C.c_size_t(n), C.byref(comb)), "verify_batch_rlc")
    return ok.astype(bool), bitmap, comb.value


def g2pubs_verify_batch_rlc(msgs, pks, sigs, inf_flags=None, scalars=None):
    """blsmi_g2pubs_verify_batch_rlc -> (ok, bitmap, combined): verify_batch's verdicts from one combined pairing check (combined == 1)
    or, when it fails, from the per-tuple path (combined == 0).  scalars: n nonzero 64-bit integers, or None (the library draws them)."""
    return _verify_batch_rlc(_lib().blsmi_g2pubs_verify_batch_rlc, 192, 96, msgs, pks, sigs, inf_flags, scalars)


def g1pubs_verify_batch_rlc(msgs, pks, sigs, inf_flags=None, scalars=None):
    return _verify_batch_rlc(_lib().blsmi_g1pubs_verify_batch_rlc, 96, 192, msgs, pks, sigs, inf_flags, scalars)


def g1pubs_verify_with_domain_batch_rlc(msgs32, domain8, pks, sigs, inf_flags=None, scalars=None):
    """-> (ok, combined)"""
    n = len(msgs32)
    buf = _u8(b"".join(bytes(m) for m in msgs32), 32 * n)
    d, p, s = _u8(domain8, 8), _u8(pks, 96 * n), _u8(sigs, 192 * n)
    f = _u8(inf_flags, n) if inf_flags is not None else None
    r, pr = _scalars(scalars, n)
    ok = np.zeros(n, dtype=np.uint8)
    comb = C.c_int(0)
    _check(_lib().blsmi_g1pubs_verify_with_domain_batch_rlc(_p8(buf), _p8(d), _p8(p), _p8(s), _p8(f), pr, _p8(ok), None, C.c_size_t(n), C.byref(comb)),
           "verify_with_domain_batch_rlc")
    return ok.astype(bool), comb.value


def verify_serialized_batch(group, msgs, pks, sigs, check_subgroup=True):
    """Deserialize + Verify in one device pass: compressed keys / signatures as Serialize() emits them.
    Returns (ok, err_pk, err_sig); err_* are the per-element deserialisation error codes (0 = fine)."""
    n = len(msgs)
    buf, off = _msgs(msgs)
    pkc, sgc = (96, 48) if group == "g2pubs" else (48, 96)
    p = _u8(pks, pkc * n) if n else np.zeros(1, np.uint8)
    s = _u8(sigs, sgc * n) if n else np.zeros(1, np.uint8)
    ok = np.zeros(n, dtype=np.uint8); ep = np.zeros(n, dtype=np.uint8); es = np.zeros(n, dtype=np.uint8)
    fn = _lib().blsmi_g2pubs_verify_serialized_batch if group == "g2pubs" else _lib().blsmi_g1pubs_verify_serialized_batch
    _check(fn(_p8(buf), off.ctypes.data_as(_u64p), _p8(p), _p8(s), C.c_int(1 if check_subgroup else 0), _p8(ok), _p8(ep), _p8(es), C.c_size_t(n)), "verify_serialized_batch")
    return ok.astype(bool), ep, es


def g1pubs_verify_with_domain_batch(msgs32, domain8, pks, sigs, inf_flags=None):
    n = len(msgs32)
    buf = _u8(b"".join(bytes(m) for m in msgs32), 32 * n)
    d, p, s = _u8(domain8, 8), _u8(pks, 96 * n), _u8(sigs, 192 * n)
    f = _u8(inf_flags, n) if inf_flags is not None else None
    ok = np.zeros(n, dtype=np.uint8)
    _check(_lib().blsmi_g1pubs_verify_with_domain_batch(_p8(buf), _p8(d), _p8(p), _p8(s), _p8(f), _p8(ok), None, C.c_size_t(n)), "verify_with_domain_batch")
    return ok.astype(bool)


def _verify_aggregate(fn, pkb, sgb, msgs, pks, sig):
    n = len(msgs)
    buf, off = _msgs(msgs)
    p = _u8(pks, pkb * n) if n else np.zeros(1, np.uint8)
    s = _u8(sig, sgb)
    ok = C.c_int(0)
    _check(fn(_p8(buf), off.ctypes.data_as(_u64p), _p8(p), _p8(s), C.c_size_t(n), C.byref(ok)), "verify_aggregate")
    return bool(ok.value)


def g2pubs_verify_aggregate(msgs, pks, sig):
    return _verify_aggregate(_lib().blsmi_g2pubs_verify_aggregate, 192, 96, msgs, pks, sig)


def g1pubs_verify_aggregate(msgs, pks, sig):
    return _verify_aggregate(_lib().blsmi_g1pubs_verify_aggregate, 96, 192, msgs, pks, sig)


def g1pubs_verify_aggregate_with_domain(msgs32, domain8, pks, sig):
    n = len(msgs32)
    buf = _u8(b"".join(bytes(m) for m in msgs32), 32 * n) if n else np.zeros(1, np.uint8)
    d, p, s = _u8(domain8, 8), (_u8(pks, 96 * n) if n else np.zeros(1, np.uint8)), _u8(sig, 192)
    ok = C.c_int(0)
    _check(_lib().blsmi_g1pubs_verify_aggregate_with_domain(_p8(buf), _p8(d), _p8(p), _p8(s), C.c_size_t(n), C.byref(ok)), "verify_aggregate_with_domain")
    return bool(ok.value)


def _verify_aggregate_common(fn, pkb, sgb, msg, pks, sig, n):
    m = _u8(bytes(msg) or b"\0")
    p = _u8(pks, pkb * n) if n else np.zeros(1, np.uint8)
    s = _u8(sig, sgb)
    ok = C.c_int(0)
    _check(fn(_p8(m), C.c_size_t(len(msg)), _p8(p), _p8(s), C.c_size_t(n), C.byref(ok)), "verify_aggregate_common")
    return bool(ok.value)


def g2pubs_verify_aggregate_common(msg, pks, sig, n):
    return _verify_aggregate_common(_lib().blsmi_g2pubs_verify_aggregate_common, 192, 96, msg, pks, sig, n)


def g1pubs_verify_aggregate_common(msg, pks, sig, n):
    return _verify_aggregate_common(_lib().blsmi_g1pubs_verify_aggregate_common, 96, 192, msg, pks, sig, n)


def g1pubs_verify_aggregate_common_with_domain(msg32, domain8, pks, sig, n):
    m, d = _u8(msg32, 32), _u8(domain8, 8)
    p = _u8(pks, 96 * n) if n else np.zeros(1, np.uint8)
    s = _u8(sig, 192)
    ok = C.c_int(0)
    _check(_lib().blsmi_g1pubs_verify_aggregate_common_with_domain(_p8(m), _p8(d), _p8(p), _p8(s), C.c_size_t(n), C.byref(ok)), "verify_aggregate_common_with_domain")
    return bool(ok.value)


def aggregate_partial(group, msgs, pks):
    """Shard-level half of VerifyAggregate: (prod_i MillerLoop(H(m_i), pk_i) as (72,) uint64 in the wire format,
    True if some key was the point at infinity)."""
    n = len(msgs)
    buf, off = _msgs(msgs)
    pkb = 192 if group == "g2pubs" else 96
    p = _u8(pks, pkb * n) if n else np.zeros(1, np.uint8)
    out = np.zeros(72, dtype=np.uint64)
    bad = C.c_int(0)
    fn = _lib().blsmi_g2pubs_aggregate_partial if group == "g2pubs" else _lib().blsmi_g1pubs_aggregate_partial
    _check(fn(_p8(buf), off.ctypes.data_as(_u64p), _p8(p), C.c_size_t(n), out.ctypes.data_as(_u64p), C.byref(bad)), "aggregate_partial")
    return out, bool(bad.value)


def fq12_product(vals):
    x = np.ascontiguousarray(vals, dtype=np.uint64).reshape(-1, 72)
    out = np.zeros(72, dtype=np.uint64)
    _check(_lib().blsmi_fq12_product(x.ctypes.data_as(_u64p), C.c_size_t(x.shape[0]), out.ctypes.data_as(_u64p)), "fq12_product")
    return out


# ---- wire format -----------------------------------------------------------------------------------
def _decompress(fn, ib, ob, data, n, check):
    a = _u8(data, ib * n)
    out = np.zeros((n, ob), dtype=np.uint8)
    inf = np.zeros(n, dtype=np.uint8)
    err = np.zeros(n, dtype=np.uint8)
    _check(fn(_p8(a), C.c_int(int(check)), _p8(out.reshape(-1)), _p8(inf), _p8(err), C.c_size_t(n)), "decompress")
    return out, inf.astype(bool), err


def g1_decompress_batch(data, n, check_subgroup=True):
    return _decompress(_lib().blsmi_g1_decompress_batch, 48, 96, data, n, check_subgroup)


def g2_decompress_batch(data, n, check_subgroup=True):
    return _decompress(_lib().blsmi_g2_decompress_batch, 96, 192, data, n, check_subgroup)


def _compress(fn, ib, ob, pts, n, in_inf):
    a = _u8(pts, ib * n)
    f = _u8(in_inf, n) if in_inf is not None else None
    out = np.zeros((n, ob), dtype=np.uint8)
    _check(fn(_p8(a), _p8(f), _p8(out.reshape(-1)), C.c_size_t(n)), "compress")
    return out


def g1_compress_batch(pts, n, in_inf=None):
    return _compress(_lib().blsmi_g1_compress_batch, 96, 48, pts, n, in_inf)


def g2_compress_batch(pts, n, in_inf=None):
    return _compress(_lib().blsmi_g2_compress_batch, 192, 96, pts, n, in_inf)


# ---- unit-level device ops (parity tests) -------------------------------------------------------------
OPS = dict(FQ_MUL=1, FQ_SQR=2, FQ_ADD=3, FQ_SUB=4, FQ_NEG=5, FQ_INV=6, FQ_SQRT=7, FQ_DBL=8, FQ_CMP=9, FQ_PARITY=10,
           FQ2_MUL=16, FQ2_SQR=17, FQ2_INV=18, FQ2_MUL_NR=19, FQ2_SQRT=20, FQ2_SQRT_ANY=21, FQ2_PARITY=22,
           FQ6_MUL=32, FQ6_SQR=33, FQ6_INV=34, FQ6_FROB1=35, FQ6_MUL_BY_1=36, FQ6_MUL_BY_01=37,
           FQ12_MUL=48, FQ12_SQR=49, FQ12_INV=50, FQ12_FROB1=51, FQ12_FROB2=52, FQ12_FROB3=53, FQ12_CYCLO_SQR=54, FQ12_CYCLO_RUN16=55,
           FQ12_MUL_BY_014=56, FQ12_MUL_BY_LINE_PAIR=57, FQ12_FINAL_EXP=58,
           G1_DOUBLE=64, G1_ADD=65, G2_DOUBLE=66, G2_ADD=67, SWU_G1=68, SWU_G2=69, G1_MUL_U64=70,
           ROW_DBL_STEP=80, ROW_DBL_STEP_REF=81, ROW_ADD_STEP=82, ROW_ADD_STEP_REF=83, ROW_G2_DOUBLE=84, ROW_G2_ADD=85, ROW_CLEAR_H2=86)


LANE_PAIR = 0x100


def debug_g2_prepare(g2_aff=None, mode=0):
    """G2AffineToPrepared of one point -> (68, 3, 12) uint64.  mode 0 / 1: computed by the one-tuple-per-lane / lane-pair
    steps; mode 2: the generator table the library prepared at start-up."""
    out = np.zeros(68 * 3 * 12, dtype=np.uint64)
    q = _u8(g2_aff, 192) if g2_aff is not None else None
    _check(_lib().blsmi_debug_g2_prepare(_p8(q), C.c_int(mode), out.ctypes.data_as(_u64p)), "blsmi_debug_g2_prepare")
    return out.reshape(68, 3, 12)


def debug_hash_tail(kind, pts, n):
    """the level program behind a small-batch hash: mapped points -> (hash points (n, 96|192) uint8, good (n,) uint8)"""
    rec, hb = (384 if kind == 1 else 192), (96 if kind == 0 else 192)
    p = _u8(pts, rec * n)
    out = np.zeros((n, hb), dtype=np.uint8); good = np.zeros(n, dtype=np.uint8)
    _check(_lib().blsmi_debug_hash_tail(C.c_int(kind), _p8(p), _p8(out.reshape(-1)), _p8(good), C.c_size_t(n)), "blsmi_debug_hash_tail")
    return out, good


def debug_hash_redo(kind, msgs, good, out, domain8=None):
    """re-hash the messages whose good byte is 0 into `out` (n, 96|192) uint8; returns the updated array"""
    n = len(msgs)
    hb = 96 if kind == 0 else 192
    o = np.ascontiguousarray(out, dtype=np.uint8).reshape(n, hb).copy()
    g = _u8(good, n)
    if kind == 2:
        buf = _u8(b"".join(bytes(m) for m in msgs), 32 * n); off = _u8(domain8, 8)
        offp = off.ctypes.data_as(_u64p)
    else:
        buf, off = _msgs(msgs)
        offp = off.ctypes.data_as(_u64p)
    _check(_lib().blsmi_debug_hash_redo(C.c_int(kind), _p8(buf), offp, _p8(g), _p8(o.reshape(-1)), C.c_size_t(n)), "blsmi_debug_hash_redo")
    return o


def debug_lat_unit(which, in_raw, nout):
    """one launch of unit program `which` of the latency path (gen_lat.py: UNIT_PROGRAMS) on (n, nin, 15) int32 raw limbs ->
    (the nout results as the kernel left them, (n, nout, 15) int32; the verdict bytes (n,) uint8).  nout = 0: a verdict program"""
    a = np.ascontiguousarray(in_raw, dtype=np.int32)
    n, nin, nl = a.shape
    assert nl == 15
    out = np.zeros((nout, 15, n), dtype=np.int32)                    # as K_OUTRAW12 writes them: structure of arrays over the tuples
    ok = np.zeros(n, dtype=np.uint8)
    i32p = C.POINTER(C.c_int32)
    _check(_lib().blsmi_debug_lat_unit(C.c_int(which), a.ctypes.data_as(i32p), C.c_size_t(nin), C.c_size_t(n), out.ctypes.data_as(i32p) if nout else None, _p8(ok)), "blsmi_debug_lat_unit")
    return np.ascontiguousarray(out.transpose(2, 0, 1)), ok


LANE_QUAD = 0x200          # BLSMI_OP_LANE_QUAD
LANE_ROW = 0x400           # BLSMI_OP_LANE_ROW


def debug_op(name, a, b=None, lane_pair=False, raw_flag=False, lane_quad=False, lane_row=False):
    op = OPS[name]
    width = 1 if op < 16 else 2 if op < 32 else 6 if op < 48 else 12 if op < 64 or op >= 80 else (3 if op in (64, 65, 68, 70) else 6)
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 6 * width)
    n = a.shape[0]
    out = np.zeros_like(a)
    flag = np.zeros(n, dtype=np.uint8)
    bp = None
    if b is not None:
        b = np.ascontiguousarray(b, dtype=np.uint64).reshape(-1, 6 * width)
        assert b.shape == a.shape
        bp = b.ctypes.data_as(_u64p)
    _check(_lib().blsmi_debug_op(op | (LANE_PAIR if lane_pair else 0) | (LANE_QUAD if lane_quad else 0) | (LANE_ROW if lane_row else 0), a.ctypes.data_as(_u64p), bp, out.ctypes.data_as(_u64p), _p8(flag), C.c_size_t(n)), "blsmi_debug_op")
    return out, (flag.copy() if raw_flag else flag.astype(bool))


# ---- the reference's in-memory points at the boundary (blsmi 0.6, include/blsmi.h "in-memory points") ------------------------
# bls.G1Projective = 18 x u64, bls.G2Projective = 36 x u64 (x, y, z; each FQ 6 little-endian u64 Montgomery limbs): 144 / 288 bytes.
G1_JAC_BYTES, G2_JAC_BYTES = 144, 288


def _j64(x, nbytes):
    a = _u8(x, nbytes) if nbytes else np.zeros(8, np.uint8)
    return a, a.ctypes.data_as(_u64p)


def _jac_to_affine(fn, jb, wb, jac, n):
    a, pa = _j64(jac, jb * n)
    out = np.zeros(max(1, wb * n), dtype=np.uint8)
    inf = np.zeros(max(1, n), dtype=np.uint8)
    _check(fn(pa, _p8(out), _p8(inf), C.c_size_t(n)), "jac_to_affine_batch")
    return out[:wb * n].tobytes(), inf[:n].astype(bool)


def g1_jac_to_affine_batch(jac, n):
    """G1Projective.ToAffine().SerializeBytes() for n in-memory points -> (n*96 wire bytes, infinity flags)"""
    return _jac_to_affine(_lib().blsmi_g1_jac_to_affine_batch, 144, 96, jac, n)


def g2_jac_to_affine_batch(jac, n):
    return _jac_to_affine(_lib().blsmi_g2_jac_to_affine_batch, 288, 192, jac, n)


def pairing_batch_jac(g1_jac, g2_jac, n):
    """bls.Pairing on n (G1Projective, G2Projective) pairs as the Go heap holds them -> (n, 72) uint64"""
    a, pa = _j64(g1_jac, 144 * n)
    b, pb = _j64(g2_jac, 288 * n)
    out = np.zeros((n, 72), dtype=np.uint64)
    _check(_lib().blsmi_pairing_batch_jac(pa, pb, out.ctypes.data_as(_u64p), C.c_size_t(n)), "blsmi_pairing_batch_jac")
    return out


def _sum_jac(fn, jb, pts, n):
    a, pa = _j64(pts, jb * n)
    out = np.zeros(jb // 8, dtype=np.uint64)
    oinf = C.c_int(0)
    _check(fn(pa, C.c_size_t(n), out.ctypes.data_as(_u64p), C.byref(oinf)), "sum_jac")
    return out.tobytes(), bool(oinf.value)


def g1_sum_jac(pts, n):
    """sum of n in-memory G1 points -> (the sum as an in-memory point with z = 1, is_infinity)"""
    return _sum_jac(_lib().blsmi_g1_sum_jac, 144, pts, n)


def g2_sum_jac(pts, n):
    return _sum_jac(_lib().blsmi_g2_sum_jac, 288, pts, n)


def _verify_batch_jac(fn, pkb, sgb, msgs, pks, sigs):
    n = len(msgs)
    buf, off = _msgs(msgs)
    p, pp = _j64(pks, pkb * n)
    s, ps = _j64(sigs, sgb * n)
    ok = np.zeros(n, dtype=np.uint8)
    bitmap = np.zeros((n + 7) // 8, dtype=np.uint8)
    _check(fn(_p8(buf), off.ctypes.data_as(_u64p), pp, ps, _p8(ok), _p8(bitmap), C.c_size_t(n)), "verify_batch_jac")
    return ok.astype(bool), bitmap


def g2pubs_verify_batch_jac(msgs, pks, sigs):
    return _verify_batch_jac(_lib().blsmi_g2pubs_verify_batch_jac, 288, 144, msgs, pks, sigs)


def g1pubs_verify_batch_jac(msgs, pks, sigs):
    return _verify_batch_jac(_lib().blsmi_g1pubs_verify_batch_jac, 144, 288, msgs, pks, sigs)


def g1pubs_verify_with_domain_batch_jac(msgs32, domain8, pks, sigs):
    n = len(msgs32)
    buf = _u8(b"".join(bytes(m) for m in msgs32), 32 * n)
    d = _u8(domain8, 8)
    p, pp = _j64(pks, 144 * n)
    s, ps = _j64(sigs, 288 * n)
    ok = np.zeros(n, dtype=np.uint8)
    _check(_lib().blsmi_g1pubs_verify_with_domain_batch_jac(_p8(buf), _p8(d), pp, ps, _p8(ok), None, C.c_size_t(n)), "verify_with_domain_batch_jac")
    return ok.astype(bool)


def _verify_batch_rlc_jac(fn, pkb, sgb, msgs, pks, sigs, scalars):
    n = len(msgs)
    buf, off = _msgs(msgs)
    p, pp = _j64(pks, pkb * n)
    s, ps = _j64(sigs, sgb * n)
    r, pr = _scalars(scalars, n)
    ok = np.zeros(n, dtype=np.uint8)
    bitmap = np.zeros((n + 7) // 8, dtype=np.uint8)
    comb = C.c_int(0)
    _check(fn(_p8(buf), off.ctypes.data_as(_u64p), pp, ps, pr, _p8(ok), _p8(bitmap), C.c_size_t(n), C.byref(comb)), "verify_batch_rlc_jac")
    return ok.astype(bool), bitmap, comb.value


def g2pubs_verify_batch_rlc_jac(msgs, pks, sigs, scalars=None):
    """blsmi_g2pubs_verify_batch_rlc_jac over in-memory points -> (ok, bitmap, combined)"""
    return _verify_batch_rlc_jac(_lib().blsmi_g2pubs_verify_batch_rlc_jac, 288, 144, msgs, pks, sigs, scalars)


def g1pubs_verify_batch_rlc_jac(msgs, pks, sigs, scalars=None):
    return _verify_batch_rlc_jac(_lib().blsmi_g1pubs_verify_batch_rlc_jac, 144, 288, msgs, pks, sigs, scalars)


def g1pubs_verify_with_domain_batch_rlc_jac(msgs32, domain8, pks, sigs, scalars=None):
    """-> (ok, combined)"""
    n = len(msgs32)
    buf = _u8(b"".join(bytes(m) for m in msgs32), 32 * n)
    d = _u8(domain8, 8)
    p, pp = _j64(pks, 144 * n)
    s, ps = _j64(sigs, 288 * n)
    r, pr = _scalars(scalars, n)
    ok = np.zeros(n, dtype=np.uint8)
    comb = C.c_int(0)
    _check(_lib().blsmi_g1pubs_verify_with_domain_batch_rlc_jac(_p8(buf), _p8(d), pp, ps, pr, _p8(ok), None, C.c_size_t(n), C.byref(comb)), "verify_with_domain_batch_rlc_jac")
    return ok.astype(bool), comb.value


def _verify_aggregate_jac(fn, pkb, sgb, msgs, pks, sig):
    n = len(msgs)
    buf, off = _msgs(msgs)
    p, pp = _j64(pks, pkb * n)
    s, ps = _j64(sig, sgb)
    ok = C.c_int(0)
    _check(fn(_p8(buf), off.ctypes.data_as(_u64p), pp, ps, C.c_size_t(n), C.byref(ok)), "verify_aggregate_jac")
    return bool(ok.value)


def g2pubs_verify_aggregate_jac(msgs, pks, sig):
    return _verify_aggregate_jac(_lib().blsmi_g2pubs_verify_aggregate_jac, 288, 144, msgs, pks, sig)


def g1pubs_verify_aggregate_jac(msgs, pks, sig):
    return _verify_aggregate_jac(_lib().blsmi_g1pubs_verify_aggregate_jac, 144, 288, msgs, pks, sig)


def g1pubs_verify_aggregate_with_domain_jac(msgs32, domain8, pks, sig):
    n = len(msgs32)
    buf = _u8(b"".join(bytes(m) for m in msgs32), 32 * n) if n else np.zeros(1, np.uint8)
    d = _u8(domain8, 8)
    p, pp = _j64(pks, 144 * n)
    s, ps = _j64(sig, 288)
    ok = C.c_int(0)
    _check(_lib().blsmi_g1pubs_verify_aggregate_with_domain_jac(_p8(buf), _p8(d), pp, ps, C.c_size_t(n), C.byref(ok)), "verify_aggregate_with_domain_jac")
    return bool(ok.value)


def _verify_aggregate_common_jac(fn, pkb, sgb, msg, pks, sig, n):
    m = _u8(bytes(msg) or b"\0")
    p, pp = _j64(pks, pkb * n)
    s, ps = _j64(sig, sgb)
    ok = C.c_int(0)
    _check(fn(_p8(m), C.c_size_t(len(msg)), pp, ps, C.c_size_t(n), C.byref(ok)), "verify_aggregate_common_jac")
    return bool(ok.value)


def g2pubs_verify_aggregate_common_jac(msg, pks, sig, n):
    return _verify_aggregate_common_jac(_lib().blsmi_g2pubs_verify_aggregate_common_jac, 288, 144, msg, pks, sig, n)


def g1pubs_verify_aggregate_common_jac(msg, pks, sig, n):
    return _verify_aggregate_common_jac(_lib().blsmi_g1pubs_verify_aggregate_common_jac, 144, 288, msg, pks, sig, n)


def g1pubs_verify_aggregate_common_with_domain_jac(msg32, domain8, pks, sig, n):
    m, d = _u8(msg32, 32), _u8(domain8, 8)
    p, pp = _j64(pks, 144 * n)
    s, ps = _j64(sig, 288)
    ok = C.c_int(0)
    _check(_lib().blsmi_g1pubs_verify_aggregate_common_with_domain_jac(_p8(m), _p8(d), pp, ps, C.c_size_t(n), C.byref(ok)), "verify_aggregate_common_with_domain_jac")
    return bool(ok.value)


class PreparedKeysJac(PreparedKeys):
    """PreparedKeys made from n in-memory G2 points (blsmi_g2_prepared_create_jac)"""

    def __init__(self, g2_jac, n):  # (does not call the affine constructor)
        a, pa = _j64(g2_jac, 288 * n)
        h = C.c_void_p(0)
        _check(_lib().blsmi_g2_prepared_create_jac(pa, C.c_size_t(n), C.byref(h)), "blsmi_g2_prepared_create_jac")
        self.ptr, self.n = h.value, n


def g2pubs_verify_batch_prepared_jac(msgs, prepared, key_idx, sigs):
    """g2pubs.Verify x n over prepared keys, the signatures as in-memory G1 points"""
    n = len(msgs)
    buf, off = _msgs(msgs)
    ptr = prepared.ptr if isinstance(prepared, PreparedKeys) else prepared
    s, ps = _j64(sigs, 144 * n)
    idx = None if key_idx is None else np.ascontiguousarray(key_idx, dtype=np.uint32)
    ok = np.zeros(n, dtype=np.uint8)
    _check(_lib().blsmi_g2pubs_verify_batch_prepared_jac(_p8(buf), off.ctypes.data_as(_u64p), C.c_void_p(ptr), None if idx is None else idx.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                        ps, _p8(ok), None, C.c_size_t(n)), "verify_batch_prepared_jac")
    return ok.astype(bool)


def g2pubs_verify_aggregate_prepared_jac(msgs, prepared, key_idx, sig):
    n = len(msgs)
    buf, off = _msgs(msgs)
    ptr = prepared.ptr if isinstance(prepared, PreparedKeys) else prepared
    s, ps = _j64(sig, 144)
    idx = None if key_idx is None else np.ascontiguousarray(key_idx, dtype=np.uint32)
    ok = C.c_int(0)
    _check(_lib().blsmi_g2pubs_verify_aggregate_prepared_jac(_p8(buf), off.ctypes.data_as(_u64p), C.c_void_p(ptr), None if idx is None else idx.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                            ps, C.c_size_t(n), C.byref(ok)), "verify_aggregate_prepared_jac")
    return bool(ok.value)


def pairing_batch_jac_dev(d_g1_jac, d_g2_jac, d_out, n, stream=0):
    _check(_lib().blsmi_pairing_batch_jac_dev(C.c_void_p(d_g1_jac), C.c_void_p(d_g2_jac), C.c_void_p(d_out), C.c_size_t(n), C.c_void_p(stream)), "blsmi_pairing_batch_jac_dev")


def verify_batch_jac_dev(group, d_msgs, d_off, d_pks_jac, d_sigs_jac, d_ok, n, stream=0):
    """group: "g2pubs" / "g1pubs" / "g1pubs_with_domain" (d_off = the 8-byte domain on the device)"""
    fn = {"g2pubs": _lib().blsmi_g2pubs_verify_batch_jac_dev, "g1pubs": _lib().blsmi_g1pubs_verify_batch_jac_dev,
          "g1pubs_with_domain": _lib().blsmi_g1pubs_verify_with_domain_batch_jac_dev}[group]
    _check(fn(C.c_void_p(d_msgs), C.c_void_p(d_off), C.c_void_p(d_pks_jac), C.c_void_p(d_sigs_jac), C.c_void_p(d_ok), C.c_size_t(n), C.c_void_p(stream)), "verify_batch_jac_dev")


def _mul_gen_jac(fn, jb, scalars, n):
    sc = _u8(scalars, 32 * n)
    out = np.zeros(max(1, jb // 8 * n), dtype=np.uint64)
    _check(fn(_p8(sc), out.ctypes.data_as(_u64p), C.c_size_t(n)), "mul_generator_batch_jac")
    return out[:jb // 8 * n].view(np.uint8).reshape(n, jb)


def g1_mul_generator_batch_jac(scalars, n):
    """PrivToPub for g1pubs: k_i * G1 as (n, 144) bytes of bls.G1Projective records (z = 1; (0, 1, 0) for k = 0 mod r)"""
    return _mul_gen_jac(_lib().blsmi_g1_mul_generator_batch_jac, 144, scalars, n)


def g2_mul_generator_batch_jac(scalars, n):
    return _mul_gen_jac(_lib().blsmi_g2_mul_generator_batch_jac, 288, scalars, n)


def _sign_jac(fn, jb, n, head, sks):
    sk = _u8(sks, 32 * n)
    out = np.zeros(max(1, jb // 8 * n), dtype=np.uint64)
    _check(fn(*head, _p8(sk), out.ctypes.data_as(_u64p), C.c_size_t(n)), "sign_batch_jac")
    return out[:jb // 8 * n].view(np.uint8).reshape(n, jb)


def g2pubs_sign_batch_jac(msgs, sks):
    buf, off = _msgs(msgs)
    return _sign_jac(_lib().blsmi_g2pubs_sign_batch_jac, 144, len(msgs), (_p8(buf), off.ctypes.data_as(_u64p)), sks)


def g1pubs_sign_batch_jac(msgs, sks):
    buf, off = _msgs(msgs)
    return _sign_jac(_lib().blsmi_g1pubs_sign_batch_jac, 288, len(msgs), (_p8(buf), off.ctypes.data_as(_u64p)), sks)


def g1pubs_sign_with_domain_batch_jac(msgs32, domain8, sks):
    n = len(msgs32)
    buf = _u8(b"".join(bytes(m) for m in msgs32), 32 * n)
    d = _u8(domain8, 8)
    return _sign_jac(_lib().blsmi_g1pubs_sign_with_domain_batch_jac, 288, n, (_p8(buf), _p8(d)), sks)


# ---- committees (blsmi 0.9): segmented sums and batches of VerifyAggregateCommon ------------------------------------------------
def seg_offsets(sizes):
    """Segment sizes -> the m + 1 offsets (uint64) of the segmented entry points: [0, s0, s0 + s1, ...]"""
    off = np.zeros(len(sizes) + 1, dtype=np.uint64)
    if len(sizes):
        np.cumsum(np.asarray(sizes, dtype=np.uint64), out=off[1:])
    return off


def _seg_args(idx, seg_off):
    so = np.ascontiguousarray(seg_off, dtype=np.uint64)
    ix = None if idx is None else np.ascontiguousarray(idx, dtype=np.uint32)
    return so, (ix.ctypes.data_as(C.POINTER(C.c_uint32)) if ix is not None and ix.size else None), ix


def _sum_segmented(fn, pb, rec, pts, npk, idx, seg_off, in_inf=None):
    so, pidx, _keep = _seg_args(idx, seg_off)
    m = so.size - 1
    if rec == pb:
        p = _u8(pts, pb * npk) if npk else np.zeros(1, np.uint8)
        pp = _p8(p)
    else:
        p, pp = _j64(pts, rec * npk)
    f = _u8(in_inf, npk) if in_inf is not None else None
    out = np.zeros(max(1, pb * m), dtype=np.uint8)
    oinf = np.zeros(max(1, m), dtype=np.uint8)
    args = (pp, _p8(f), C.c_size_t(npk)) if rec == pb else (pp, C.c_size_t(npk))
    _check(fn(*args, pidx, so.ctypes.data_as(_u64p), C.c_size_t(m), _p8(out), _p8(oinf)), "sum_segmented")
    return out[:pb * m].tobytes(), oinf[:m].copy()


def g1_sum_segmented(pts, npk, idx, seg_off, in_inf=None):
    """m sums of affine G1 points: segment j = pts[idx[k]] for seg_off[j] <= k < seg_off[j + 1] (idx None: k itself).
    -> (m*96 affine bytes, out_inf: 1 infinity, 0 otherwise)"""
    return _sum_segmented(_lib().blsmi_g1_sum_segmented, 96, 96, pts, npk, idx, seg_off, in_inf)


def g2_sum_segmented(pts, npk, idx, seg_off, in_inf=None):
    return _sum_segmented(_lib().blsmi_g2_sum_segmented, 192, 192, pts, npk, idx, seg_off, in_inf)


def g1_sum_segmented_jac(pts_jac, npk, idx, seg_off):
    """the same over in-memory G1 points (144 bytes each) -> affine records and flags"""
    return _sum_segmented(_lib().blsmi_g1_sum_segmented_jac, 96, 144, pts_jac, npk, idx, seg_off)


def g2_sum_segmented_jac(pts_jac, npk, idx, seg_off):
    return _sum_segmented(_lib().blsmi_g2_sum_segmented_jac, 192, 288, pts_jac, npk, idx, seg_off)


def sum_segmented_dev(group, d_pts, d_in_inf, npk, d_idx, d_seg_off, m, d_out, d_out_inf, stream=0):
    """device-pointer form: out_inf bytes 0 / 1 / 2 (2: the segment holds an index >= npk, record zeroed)"""
    fn = _lib().blsmi_g1_sum_segmented_dev if group == "g1" else _lib().blsmi_g2_sum_segmented_dev
    _check(fn(C.c_void_p(d_pts or 0), C.c_void_p(d_in_inf or 0), C.c_size_t(npk), C.c_void_p(d_idx or 0), C.c_void_p(d_seg_off or 0), C.c_size_t(m),
              C.c_void_p(d_out or 0), C.c_void_p(d_out_inf or 0), C.c_void_p(stream)), "sum_segmented_dev")


def _agg_common_batch(fn, name, pkb, sgb, jac, head, pks, npk, idx, seg_off, sigs):
    so, pidx, _keep = _seg_args(idx, seg_off)
    m = so.size - 1
    if jac:
        p, pp = _j64(pks, pkb * npk)
        s, ps = _j64(sigs, sgb * m)
    else:
        p = _u8(pks, pkb * npk) if npk else np.zeros(1, np.uint8)
        s = _u8(sigs, sgb * m) if m else np.zeros(1, np.uint8)
        pp, ps = _p8(p), _p8(s)
    ok = np.zeros(max(1, m), dtype=np.uint8)
    bm = np.zeros(max(1, (m + 7) // 8), dtype=np.uint8)
    _check(fn(*head, pp, C.c_size_t(npk), pidx, so.ctypes.data_as(_u64p), ps, _p8(ok), _p8(bm), C.c_size_t(m)), name)
    return ok[:m].copy(), bm[:(m + 7) // 8].copy()


def _msg_head(msgs):
    buf, off = _msgs(msgs)
    return (buf, off), (_p8(buf), off.ctypes.data_as(_u64p))


def g2pubs_verify_aggregate_common_batch(msgs, pks, npk, idx, seg_off, sigs):
    """item j: VerifyAggregateCommon(sigs[j], {pks[idx[k]] : seg_off[j] <= k < seg_off[j + 1]}, msgs[j]) -> (m verdict bytes, bitmap)"""
    mm, head = _msg_head(msgs)
    return _agg_common_batch(_lib().blsmi_g2pubs_verify_aggregate_common_batch, "g2pubs_verify_aggregate_common_batch", 192, 96, False, head, pks, npk, idx, seg_off, sigs)


def g1pubs_verify_aggregate_common_batch(msgs, pks, npk, idx, seg_off, sigs):
    mm, head = _msg_head(msgs)
    return _agg_common_batch(_lib().blsmi_g1pubs_verify_aggregate_common_batch, "g1pubs_verify_aggregate_common_batch", 96, 192, False, head, pks, npk, idx, seg_off, sigs)


def g1pubs_verify_aggregate_common_with_domain_batch(msgs32, domain8, pks, npk, idx, seg_off, sigs):
    m = len(seg_off) - 1
    buf, d = _u8(msgs32, 32 * m) if m else np.zeros(1, np.uint8), _u8(domain8, 8)
    return _agg_common_batch(_lib().blsmi_g1pubs_verify_aggregate_common_with_domain_batch, "g1pubs_verify_aggregate_common_with_domain_batch", 96, 192, False,
                             (_p8(buf), _p8(d)), pks, npk, idx, seg_off, sigs)


def g2pubs_verify_aggregate_common_batch_jac(msgs, pks, npk, idx, seg_off, sigs):
    """the same over in-memory keys (288 bytes) and signatures (144 bytes)"""
    mm, head = _msg_head(msgs)
    return _agg_common_batch(_lib().blsmi_g2pubs_verify_aggregate_common_batch_jac, "g2pubs_verify_aggregate_common_batch_jac", 288, 144, True, head, pks, npk, idx, seg_off, sigs)


def g1pubs_verify_aggregate_common_batch_jac(msgs, pks, npk, idx, seg_off, sigs):
    mm, head = _msg_head(msgs)
    return _agg_common_batch(_lib().blsmi_g1pubs_verify_aggregate_common_batch_jac, "g1pubs_verify_aggregate_common_batch_jac", 144, 288, True, head, pks, npk, idx, seg_off, sigs)


def g1pubs_verify_aggregate_common_with_domain_batch_jac(msgs32, domain8, pks, npk, idx, seg_off, sigs):
    m = len(seg_off) - 1
    buf, d = _u8(msgs32, 32 * m) if m else np.zeros(1, np.uint8), _u8(domain8, 8)
    return _agg_common_batch(_lib().blsmi_g1pubs_verify_aggregate_common_with_domain_batch_jac, "g1pubs_verify_aggregate_common_with_domain_batch_jac", 144, 288, True,
                             (_p8(buf), _p8(d)), pks, npk, idx, seg_off, sigs)


def verify_aggregate_common_batch_dev(group, d_msgs, d_off_or_domain, d_pks, npk, d_idx, d_seg_off, d_sigs, d_ok, m, stream=0, domain=False):
    """device-pointer forms: group "g2pubs" / "g1pubs" (domain=True: d_msgs holds m*32 bytes, d_off_or_domain the 8-byte domain); verdicts in d_ok"""
    lib = _lib()
    fn = lib.blsmi_g2pubs_verify_aggregate_common_batch_dev if group == "g2pubs" else \
        (lib.blsmi_g1pubs_verify_aggregate_common_with_domain_batch_dev if domain else lib.blsmi_g1pubs_verify_aggregate_common_batch_dev)
    _check(fn(C.c_void_p(d_msgs or 0), C.c_void_p(d_off_or_domain or 0), C.c_void_p(d_pks or 0), C.c_size_t(npk), C.c_void_p(d_idx or 0),
              C.c_void_p(d_seg_off or 0), C.c_void_p(d_sigs or 0), C.c_void_p(d_ok or 0), C.c_size_t(m), C.c_void_p(stream)), "verify_aggregate_common_batch_dev")


# ---- grouped randomised batch verification and the weighted segmented sums (blsmi 0.11) ----------------------------------------------
_u32p = C.POINTER(C.c_uint32)
_G_HEAD = [_u8p, _u64p, C.c_size_t, _u32p]                                 # msgs, msg_off, d, msg_idx
_G_HEAD_DOMAIN = [_u8p, _u8p, C.c_size_t, _u32p]                           # msgs32, domain, d, msg_idx
_G_TAIL = [_u64p, _u8p, _u8p, C.c_size_t, C.POINTER(C.c_int)]              # scalars, ok, ok_bitmap, n, combined
_SUM_U64 = [_u8p, _u8p, C.c_size_t, _u64p, _u32p, _u64p, C.c_size_t, _u8p, _u8p]
# the argument types of the eight entry points of 0.11, as include/blsmi.h declares them (tests/test_rlc_grouped_cpu.py compares)
ARGTYPES_0_11 = {
    "blsmi_g2pubs_verify_batch_rlc_grouped": _G_HEAD + [_u8p, _u8p, _u8p] + _G_TAIL,
    "blsmi_g1pubs_verify_batch_rlc_grouped": _G_HEAD + [_u8p, _u8p, _u8p] + _G_TAIL,
    "blsmi_g1pubs_verify_with_domain_batch_rlc_grouped": _G_HEAD_DOMAIN + [_u8p, _u8p, _u8p] + _G_TAIL,
    "blsmi_g2pubs_verify_batch_rlc_grouped_jac": _G_HEAD + [_u64p, _u64p] + _G_TAIL,
    "blsmi_g1pubs_verify_batch_rlc_grouped_jac": _G_HEAD + [_u64p, _u64p] + _G_TAIL,
    "blsmi_g1pubs_verify_with_domain_batch_rlc_grouped_jac": _G_HEAD_DOMAIN + [_u64p, _u64p] + _G_TAIL,
    "blsmi_g1_sum_segmented_u64": _SUM_U64,
    "blsmi_g2_sum_segmented_u64": _SUM_U64,
}


def _fn(name):
    """the entry point `name` of 0.11 and later, with the argument types its ARGTYPES_0_NN table (here and below) gives it"""
    tables = (ARGTYPES_0_11, ARGTYPES_0_12, ARGTYPES_0_13, ARGTYPES_0_14, ARGTYPES_0_15, ARGTYPES_0_16, ARGTYPES_0_17, ARGTYPES_0_18, ARGTYPES_0_19)
    fn = getattr(_lib(), name)
    fn.argtypes = next(t[name] for t in tables if name in t)
    fn.restype = C.c_int
    return fn


def _msg_idx(msg_idx, n):
    ix = np.ascontiguousarray(np.asarray(msg_idx, dtype=np.uint32))
    if ix.shape != (n,):
        raise ValueError("need one message index per tuple")
    return ix, (ix.ctypes.data_as(_u32p) if n else None)


def _rlc_marshal(kind, jac, msgs, n, pks, sigs, inf_flags, scalars, domain8):
    """The arguments the grouped and the block-locating forms pass alike, for n tuples over the messages `msgs` -> (head, mid, pr, ok, bitmap,
    comb, keep): head = the messages and their offsets (or the domain), mid = keys, signatures (and infinity flags), pr = the scalars; ok, bitmap
    and comb receive the results; keep holds the arrays the pointers refer to."""
    pkb, sgb = (192, 96) if kind == 0 else (96, 192)
    if domain8 is None:
        buf, off = _msgs(msgs)
        head = (_p8(buf), off.ctypes.data_as(_u64p))
    else:
        buf = _u8(b"".join(bytes(m) for m in msgs) or b"\0" * 32, 32 * max(len(msgs), 1))
        off = _u8(domain8, 8)
        head = (_p8(buf), _p8(off))
    if jac:
        p, pp = _j64(pks, pkb // 2 * 3 * n)
        s, ps = _j64(sigs, sgb // 2 * 3 * n)
        f = None
        mid = (pp, ps)
    else:
        p, s = _u8(pks, pkb * n), _u8(sigs, sgb * n)
        f = _u8(inf_flags, n) if inf_flags is not None else None
        mid = (_p8(p), _p8(s), _p8(f))
    r, pr = _scalars(scalars, n)
    ok = np.zeros(n, dtype=np.uint8)
    bitmap = np.zeros((n + 7) // 8, dtype=np.uint8)
    return head, mid, pr, ok, bitmap, C.c_int(0), (buf, off, p, s, f, r)


def _verify_batch_rlc_grouped(name, kind, jac, msgs, msg_idx, pks, sigs, inf_flags, scalars, domain8=None):
    """-> (ok, bitmap, combined); msgs: the table of d messages, msg_idx: n indices into it"""
    n = len(msg_idx)
    ix, pix = _msg_idx(msg_idx, n)
    head, mid, pr, ok, bitmap, comb, _keep = _rlc_marshal(kind, jac, msgs, n, pks, sigs, inf_flags, scalars, domain8)
    _check(_fn(name)(*head, len(msgs), pix, *mid, pr, _p8(ok), _p8(bitmap), n, C.byref(comb)), name[len("blsmi_"):])
    return ok.astype(bool), bitmap, comb.value


def g2pubs_verify_batch_rlc_grouped(msgs, msg_idx, pks, sigs, inf_flags=None, scalars=None):
    """blsmi_g2pubs_verify_batch_rlc_grouped -> (ok, bitmap, combined): tuple i is (msgs[msg_idx[i]], pk_i, sig_i); the tuples of one message
    share one pairing of the combined check.  Verdicts as g2pubs_verify_batch_rlc on the expanded messages."""
    return _verify_batch_rlc_grouped("blsmi_g2pubs_verify_batch_rlc_grouped", 0, False, msgs, msg_idx, pks, sigs, inf_flags, scalars)


def g1pubs_verify_batch_rlc_grouped(msgs, msg_idx, pks, sigs, inf_flags=None, scalars=None):
    return _verify_batch_rlc_grouped("blsmi_g1pubs_verify_batch_rlc_grouped", 1, False, msgs, msg_idx, pks, sigs, inf_flags, scalars)


def g1pubs_verify_with_domain_batch_rlc_grouped(msgs32, domain8, msg_idx, pks, sigs, inf_flags=None, scalars=None):
    return _verify_batch_rlc_grouped("blsmi_g1pubs_verify_with_domain_batch_rlc_grouped", 2, False, msgs32, msg_idx, pks, sigs, inf_flags, scalars, domain8)


def g2pubs_verify_batch_rlc_grouped_jac(msgs, msg_idx, pks, sigs, scalars=None):
    """the same over in-memory points (288 / 144 bytes each)"""
    return _verify_batch_rlc_grouped("blsmi_g2pubs_verify_batch_rlc_grouped_jac", 0, True, msgs, msg_idx, pks, sigs, None, scalars)


def g1pubs_verify_batch_rlc_grouped_jac(msgs, msg_idx, pks, sigs, scalars=None):
    return _verify_batch_rlc_grouped("blsmi_g1pubs_verify_batch_rlc_grouped_jac", 1, True, msgs, msg_idx, pks, sigs, None, scalars)


def g1pubs_verify_with_domain_batch_rlc_grouped_jac(msgs32, domain8, msg_idx, pks, sigs, scalars=None):
    return _verify_batch_rlc_grouped("blsmi_g1pubs_verify_with_domain_batch_rlc_grouped_jac", 2, True, msgs32, msg_idx, pks, sigs, None, scalars, domain8)


def _sum_segmented_u64(name, pb, pts, npk, scalars, idx, seg_off, in_inf):
    so, pidx, _keep = _seg_args(idx, seg_off)
    m = so.size - 1
    p = _u8(pts, pb * npk) if npk else np.zeros(1, np.uint8)
    r, pr = _scalars(scalars, npk)
    f = _u8(in_inf, npk) if in_inf is not None else None
    out = np.zeros(max(1, pb * m), dtype=np.uint8)
    oinf = np.zeros(max(1, m), dtype=np.uint8)
    _check(_fn(name)(_p8(p), _p8(f), npk, pr if npk else None, pidx, so.ctypes.data_as(_u64p), m, _p8(out), _p8(oinf)), name[len("blsmi_"):])
    return out[:pb * m].tobytes(), oinf[:m].copy()


def g1_sum_segmented_u64(pts, npk, scalars, idx, seg_off, in_inf=None):
    """m weighted sums of affine G1 points: segment j = sum scalars[idx[k]] * pts[idx[k]] for seg_off[j] <= k < seg_off[j + 1]; scalars: npk
    64-bit integers (zero allowed).  -> (m*96 affine bytes, out_inf)"""
    return _sum_segmented_u64("blsmi_g1_sum_segmented_u64", 96, pts, npk, scalars, idx, seg_off, in_inf)


def g2_sum_segmented_u64(pts, npk, scalars, idx, seg_off, in_inf=None):
    return _sum_segmented_u64("blsmi_g2_sum_segmented_u64", 192, pts, npk, scalars, idx, seg_off, in_inf)


# ---- pairing products (blsmi 0.10): many MillerLoop(items) + FinalExponentiation checks in one call -----------------------------
def _pprod_offsets(seg_off, np_):
    so = np.ascontiguousarray(seg_off, dtype=np.uint64).reshape(-1)
    if so.size < 1:
        raise ValueError("seg_off needs m + 1 entries")
    if so.size > 1 and int(so[-1]) != np_:
        raise ValueError("seg_off ends at %d, the call has %d pairs" % (int(so[-1]), np_))
    return so, so.size - 1


def _pprod_out(m):
    return np.zeros((m, 72), dtype=np.uint64), np.zeros(max(1, m), dtype=np.uint8)


def pairing_product_batch(g1_aff, g2_aff, seg_off, inf_flags=None):
    """item j = FinalExponentiation(MillerLoop({(P_k, Q_k) : seg_off[j] <= k < seg_off[j + 1]})) over affine records (96 / 192 bytes a
    point; inf_flags[k] bit 0 / 1: P_k / Q_k is the point at infinity) -> (values (m, 72) uint64, is_one (m,) uint8)"""
    a, b = _u8(g1_aff), _u8(g2_aff)
    if a.size % 96 or b.size != 2 * a.size:
        raise ValueError("expected np*96 and np*192 bytes, got %d and %d" % (a.size, b.size))
    n = a.size // 96
    so, m = _pprod_offsets(seg_off, n)
    f = _u8(inf_flags, n) if inf_flags is not None else None
    out, one = _pprod_out(m)
    _check(_lib().blsmi_pairing_product_batch(_p8(a), _p8(b), _p8(f), C.c_size_t(n), so.ctypes.data_as(_u64p), C.c_size_t(m),
                                              out.ctypes.data_as(_u64p), _p8(one)), "blsmi_pairing_product_batch")
    return out, one[:m].copy()


def pairing_product_batch_jac(g1_jac, g2_jac, seg_off):
    """the same over in-memory points (144 / 288 bytes each, z == 0: infinity)"""
    a, b = _u8(g1_jac), _u8(g2_jac)
    if a.size % 144 or b.size != 2 * a.size:
        raise ValueError("expected np*144 and np*288 bytes, got %d and %d" % (a.size, b.size))
    n = a.size // 144
    so, m = _pprod_offsets(seg_off, n)
    out, one = _pprod_out(m)
    (a, pa), (b, pb) = _j64(a, 144 * n), _j64(b, 288 * n)
    _check(_lib().blsmi_pairing_product_batch_jac(pa, pb, C.c_size_t(n), so.ctypes.data_as(_u64p), C.c_size_t(m), out.ctypes.data_as(_u64p), _p8(one)),
           "blsmi_pairing_product_batch_jac")
    return out, one[:m].copy()


def pairing_product_batch_dev(d_g1, d_g2, np_, d_seg_off, m, d_out_fq12, d_is_one, d_inf_flags=0, stream=0, jac=False):
    """device-pointer forms (ints): jac=False affine records and optional flags, jac=True in-memory points; d_out_fq12 (m*576 bytes) or
    d_is_one (m bytes) may be 0, not both"""
    v = C.c_void_p
    if jac:
        if d_inf_flags:
            raise ValueError("the in-memory form takes no flags: z == 0 is infinity")
        rc = _lib().blsmi_pairing_product_batch_jac_dev(v(d_g1 or 0), v(d_g2 or 0), C.c_size_t(np_), v(d_seg_off or 0), C.c_size_t(m), v(d_out_fq12 or 0), v(d_is_one or 0), v(stream))
    else:
        rc = _lib().blsmi_pairing_product_batch_dev(v(d_g1 or 0), v(d_g2 or 0), v(d_inf_flags or 0), C.c_size_t(np_), v(d_seg_off or 0), C.c_size_t(m),
                                                    v(d_out_fq12 or 0), v(d_is_one or 0), v(stream))
    _check(rc, "blsmi_pairing_product_batch_jac_dev" if jac else "blsmi_pairing_product_batch_dev")


# ---- randomised batch verification that finds the bad tuples by blocks (blsmi 0.12) ---------------------------------------------------
_L_TAIL = [_u64p, C.c_size_t, _u8p, _u8p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_size_t)]   # scalars, block, ok, ok_bitmap, n, combined, rechecked
# the argument types of the six entry points of 0.12, as include/blsmi.h declares them (tests/test_rlc_locate_cpu.py compares)
ARGTYPES_0_12 = {
    "blsmi_g2pubs_verify_batch_rlc_locate": [_u8p, _u64p, _u8p, _u8p, _u8p] + _L_TAIL,
    "blsmi_g1pubs_verify_batch_rlc_locate": [_u8p, _u64p, _u8p, _u8p, _u8p] + _L_TAIL,
    "blsmi_g1pubs_verify_with_domain_batch_rlc_locate": [_u8p, _u8p, _u8p, _u8p, _u8p] + _L_TAIL,
    "blsmi_g2pubs_verify_batch_rlc_locate_jac": [_u8p, _u64p, _u64p, _u64p] + _L_TAIL,
    "blsmi_g1pubs_verify_batch_rlc_locate_jac": [_u8p, _u64p, _u64p, _u64p] + _L_TAIL,
    "blsmi_g1pubs_verify_with_domain_batch_rlc_locate_jac": [_u8p, _u8p, _u64p, _u64p] + _L_TAIL,
}


def _verify_batch_rlc_locate(name, kind, jac, msgs, pks, sigs, inf_flags, scalars, block, domain8=None):
    """-> (ok, bitmap, combined, rechecked)"""
    n = len(msgs)
    block = int(block)
    if block < 0:
        raise ValueError("block must not be negative")
    head, mid, pr, ok, bitmap, comb, _keep = _rlc_marshal(kind, jac, msgs, n, pks, sigs, inf_flags, scalars, domain8)
    rechecked = C.c_size_t(0)
    _check(_fn(name)(*head, *mid, pr, block, _p8(ok), _p8(bitmap), n, C.byref(comb), C.byref(rechecked)), name[len("blsmi_"):])
    return ok.astype(bool), bitmap, comb.value, rechecked.value


def g2pubs_verify_batch_rlc_locate(msgs, pks, sigs, inf_flags=None, scalars=None, block=0):
    """blsmi_g2pubs_verify_batch_rlc_locate -> (ok, bitmap, combined, rechecked): g2pubs_verify_batch_rlc's total check; when it fails, one
    pairing equation per block of `block` tuples (0: automatic; else even, >= 2) and verify_batch's verdicts for the tuples of the failing
    blocks only -- `rechecked` of them."""
    return _verify_batch_rlc_locate("blsmi_g2pubs_verify_batch_rlc_locate", 0, False, msgs, pks, sigs, inf_flags, scalars, block)


def g1pubs_verify_batch_rlc_locate(msgs, pks, sigs, inf_flags=None, scalars=None, block=0):
    return _verify_batch_rlc_locate("blsmi_g1pubs_verify_batch_rlc_locate", 1, False, msgs, pks, sigs, inf_flags, scalars, block)


def g1pubs_verify_with_domain_batch_rlc_locate(msgs32, domain8, pks, sigs, inf_flags=None, scalars=None, block=0):
    return _verify_batch_rlc_locate("blsmi_g1pubs_verify_with_domain_batch_rlc_locate", 2, False, msgs32, pks, sigs, inf_flags, scalars, block, domain8)


def g2pubs_verify_batch_rlc_locate_jac(msgs, pks, sigs, scalars=None, block=0):
    """the same over in-memory points (288 / 144 bytes each)"""
    return _verify_batch_rlc_locate("blsmi_g2pubs_verify_batch_rlc_locate_jac", 0, True, msgs, pks, sigs, None, scalars, block)


def g1pubs_verify_batch_rlc_locate_jac(msgs, pks, sigs, scalars=None, block=0):
    return _verify_batch_rlc_locate("blsmi_g1pubs_verify_batch_rlc_locate_jac", 1, True, msgs, pks, sigs, None, scalars, block)


def g1pubs_verify_with_domain_batch_rlc_locate_jac(msgs32, domain8, pks, sigs, scalars=None, block=0):
    return _verify_batch_rlc_locate("blsmi_g1pubs_verify_with_domain_batch_rlc_locate_jac", 2, True, msgs32, pks, sigs, None, scalars, block, domain8)


# ---- grouped randomised batch verification that finds the bad tuples by cells (blsmi 0.13) ---------------------------------------------
# the argument types of the six entry points of 0.13, as include/blsmi.h declares them (tests/test_rlc_grouped_locate_cpu.py compares)
ARGTYPES_0_13 = {
    "blsmi_g2pubs_verify_batch_rlc_grouped_locate": _G_HEAD + [_u8p, _u8p, _u8p] + _L_TAIL,
    "blsmi_g1pubs_verify_batch_rlc_grouped_locate": _G_HEAD + [_u8p, _u8p, _u8p] + _L_TAIL,
    "blsmi_g1pubs_verify_with_domain_batch_rlc_grouped_locate": _G_HEAD_DOMAIN + [_u8p, _u8p, _u8p] + _L_TAIL,
    "blsmi_g2pubs_verify_batch_rlc_grouped_locate_jac": _G_HEAD + [_u64p, _u64p] + _L_TAIL,
    "blsmi_g1pubs_verify_batch_rlc_grouped_locate_jac": _G_HEAD + [_u64p, _u64p] + _L_TAIL,
    "blsmi_g1pubs_verify_with_domain_batch_rlc_grouped_locate_jac": _G_HEAD_DOMAIN + [_u64p, _u64p] + _L_TAIL,
}


def _verify_batch_rlc_grouped_locate(name, kind, jac, msgs, msg_idx, pks, sigs, inf_flags, scalars, block, domain8=None):
    """-> (ok, bitmap, combined, rechecked); msgs: the table of d messages, msg_idx: n indices into it"""
    n = len(msg_idx)
    block = int(block)
    if block < 0:
        raise ValueError("block must not be negative")
    ix, pix = _msg_idx(msg_idx, n)
    head, mid, pr, ok, bitmap, comb, _keep = _rlc_marshal(kind, jac, msgs, n, pks, sigs, inf_flags, scalars, domain8)
    rechecked = C.c_size_t(0)
    _check(_fn(name)(*head, len(msgs), pix, *mid, pr, block, _p8(ok), _p8(bitmap), n, C.byref(comb), C.byref(rechecked)), name[len("blsmi_"):])
    return ok.astype(bool), bitmap, comb.value, rechecked.value


def g2pubs_verify_batch_rlc_grouped_locate(msgs, msg_idx, pks, sigs, inf_flags=None, scalars=None, block=0):
    """blsmi_g2pubs_verify_batch_rlc_grouped_locate -> (ok, bitmap, combined, rechecked): g2pubs_verify_batch_rlc_grouped's total check over
    cells of at most `block` tuples of one message (0: automatic; else any value >= 1); when it fails, one pairing equation per cell and
    verify_batch's verdicts for the tuples of the failing cells only -- `rechecked` of them."""
    return _verify_batch_rlc_grouped_locate("blsmi_g2pubs_verify_batch_rlc_grouped_locate", 0, False, msgs, msg_idx, pks, sigs, inf_flags, scalars, block)


def g1pubs_verify_batch_rlc_grouped_locate(msgs, msg_idx, pks, sigs, inf_flags=None, scalars=None, block=0):
    return _verify_batch_rlc_grouped_locate("blsmi_g1pubs_verify_batch_rlc_grouped_locate", 1, False, msgs, msg_idx, pks, sigs, inf_flags, scalars, block)


def g1pubs_verify_with_domain_batch_rlc_grouped_locate(msgs32, domain8, msg_idx, pks, sigs, inf_flags=None, scalars=None, block=0):
    return _verify_batch_rlc_grouped_locate("blsmi_g1pubs_verify_with_domain_batch_rlc_grouped_locate", 2, False, msgs32, msg_idx, pks, sigs, inf_flags, scalars, block, domain8)


def g2pubs_verify_batch_rlc_grouped_locate_jac(msgs, msg_idx, pks, sigs, scalars=None, block=0):
    """the same over in-memory points (288 / 144 bytes each)"""
    return _verify_batch_rlc_grouped_locate("blsmi_g2pubs_verify_batch_rlc_grouped_locate_jac", 0, True, msgs, msg_idx, pks, sigs, None, scalars, block)


def g1pubs_verify_batch_rlc_grouped_locate_jac(msgs, msg_idx, pks, sigs, scalars=None, block=0):
    return _verify_batch_rlc_grouped_locate("blsmi_g1pubs_verify_batch_rlc_grouped_locate_jac", 1, True, msgs, msg_idx, pks, sigs, None, scalars, block)


def g1pubs_verify_with_domain_batch_rlc_grouped_locate_jac(msgs32, domain8, msg_idx, pks, sigs, scalars=None, block=0):
    return _verify_batch_rlc_grouped_locate("blsmi_g1pubs_verify_with_domain_batch_rlc_grouped_locate_jac", 2, True, msgs32, msg_idx, pks, sigs, None, scalars, block, domain8)


# ---- point validation (blsmi 0.14): on-curve and subgroup status of points in either form ----------------------------------------------
POINT_OK, POINT_INFINITY, POINT_NOT_ON_CURVE, POINT_NOT_IN_SUBGROUP = 0, 1, 3, 4   # BLSMI_POINT_* (3, 4: the decompression error codes)
_V = C.c_void_p
# the argument types of the six entry points of 0.14, as include/blsmi.h declares them (tests/test_point_check_cpu.py compares)
ARGTYPES_0_14 = {
    "blsmi_g1_check_batch": [_u8p, _u8p, C.c_int, _u8p, C.c_size_t],
    "blsmi_g2_check_batch": [_u8p, _u8p, C.c_int, _u8p, C.c_size_t],
    "blsmi_g1_check_batch_jac": [_u64p, C.c_int, _u8p, C.c_size_t],
    "blsmi_g2_check_batch_jac": [_u64p, C.c_int, _u8p, C.c_size_t],
    "blsmi_g1_check_batch_dev": [_V, _V, C.c_int, C.c_int, _V, C.c_size_t, _V],
    "blsmi_g2_check_batch_dev": [_V, _V, C.c_int, C.c_int, _V, C.c_size_t, _V],
}


def _check_batch(name, pb, pts, n, in_inf, check):
    a = _u8(pts, pb * n) if n else np.zeros(1, np.uint8)
    f = _u8(in_inf, n) if in_inf is not None else None
    status = np.zeros(max(1, n), dtype=np.uint8)
    _check(_fn(name)(_p8(a), _p8(f), int(check), _p8(status), n), name[len("blsmi_"):])
    return status[:n].copy()


def g1_check_batch(pts, n, in_inf=None, check=1):
    """IsOnCurve / IsInCorrectSubgroupAssumingOnCurve of n affine G1 records (96 bytes each; in_inf: optional infinity flags) -> (n,) uint8:
    0 good, 1 infinity, 3 not on the curve, 4 outside the subgroup.  check: 0 the curve equation only, 1 the endomorphism test, 2 r * P."""
    return _check_batch("blsmi_g1_check_batch", 96, pts, n, in_inf, check)


def g2_check_batch(pts, n, in_inf=None, check=1):
    return _check_batch("blsmi_g2_check_batch", 192, pts, n, in_inf, check)


def _check_batch_jac(name, jb, jac, n, check):
    a, pa = _j64(jac, jb * n)
    status = np.zeros(max(1, n), dtype=np.uint8)
    _check(_fn(name)(pa, int(check), _p8(status), n), name[len("blsmi_"):])
    return status[:n].copy()


def g1_check_batch_jac(jac, n, check=1):
    """the same over in-memory G1 points (144 bytes each, z == 0: infinity): no conversion to affine, no inversion"""
    return _check_batch_jac("blsmi_g1_check_batch_jac", 144, jac, n, check)


def g2_check_batch_jac(jac, n, check=1):
    return _check_batch_jac("blsmi_g2_check_batch_jac", 288, jac, n, check)


def check_batch_dev(group, d_pts, d_in_inf, n, d_status, jac=False, check=1, stream=0):
    """device-pointer form (ints): d_pts affine records, or in-memory points with jac=True (then d_in_inf must be 0).  The n status bytes are
    in d_status when the call returns (it synchronises); the caller's point buffers are only read."""
    if jac and d_in_inf:
        raise ValueError("the in-memory form takes no flags: z == 0 is infinity")
    name = "blsmi_g1_check_batch_dev" if group == "g1" else "blsmi_g2_check_batch_dev"
    _check(_fn(name)(d_pts or 0, d_in_inf or 0, int(bool(jac)), int(check), d_status or 0, n, stream or 0), name[len("blsmi_"):])


# ---- the wire format <-> in-memory points (blsmi 0.15) -----------------------------------------------------------------------------------
# the argument types of the eight entry points of 0.15, as include/blsmi.h declares them (tests/test_wire_jac_cpu.py compares)
ARGTYPES_0_15 = {
    "blsmi_g1_decompress_batch_jac": [_u8p, C.c_int, _u64p, _u8p, _u8p, C.c_size_t],
    "blsmi_g2_decompress_batch_jac": [_u8p, C.c_int, _u64p, _u8p, _u8p, C.c_size_t],
    "blsmi_g1_compress_batch_jac": [_u64p, _u8p, C.c_size_t],
    "blsmi_g2_compress_batch_jac": [_u64p, _u8p, C.c_size_t],
    "blsmi_g1_decompress_batch_jac_dev": [_V, C.c_int, _V, _V, _V, C.c_size_t, _V],
    "blsmi_g2_decompress_batch_jac_dev": [_V, C.c_int, _V, _V, _V, C.c_size_t, _V],
    "blsmi_g1_compress_batch_jac_dev": [_V, _V, C.c_size_t, _V],
    "blsmi_g2_compress_batch_jac_dev": [_V, _V, C.c_size_t, _V],
}


def _decompress_jac(name, ib, jb, data, n, check):
    a = _u8(data, ib * n) if n else np.zeros(1, np.uint8)
    out = np.zeros(max(1, n) * jb, dtype=np.uint8)
    inf = np.zeros(max(1, n), dtype=np.uint8)
    err = np.zeros(max(1, n), dtype=np.uint8)
    _check(_fn(name)(_p8(a), int(check), out.ctypes.data_as(_u64p), _p8(inf), _p8(err), n), name[len("blsmi_"):])
    return out[:n * jb].reshape(n, jb), inf[:n].astype(bool), err[:n].copy()


def g1_decompress_batch_jac(data, n, check_subgroup=True):
    """DecompressG1(b).ToProjective() of n 48-byte encodings -> ((n, 144) uint8 in-memory records, infinity flags, error codes); the flags and
    codes are g1_decompress_batch's, the record of an infinity or of an encoding with an error is the reference's zero point (0, 1, 0)"""
    return _decompress_jac("blsmi_g1_decompress_batch_jac", 48, 144, data, n, check_subgroup)


def g2_decompress_batch_jac(data, n, check_subgroup=True):
    return _decompress_jac("blsmi_g2_decompress_batch_jac", 96, 288, data, n, check_subgroup)


def _compress_jac(name, jb, ob, jac, n):
    a, pa = _j64(jac, jb * n)
    out = np.zeros((max(1, n), ob), dtype=np.uint8)
    _check(_fn(name)(pa, _p8(out.reshape(-1)), n), name[len("blsmi_"):])
    return out[:n]


def g1_compress_batch_jac(jac, n):
    """CompressG1(p.ToAffine()) of n in-memory G1 points (144 bytes each, z == 0: infinity) -> (n, 48) uint8, one call and one launch"""
    return _compress_jac("blsmi_g1_compress_batch_jac", 144, 48, jac, n)


def g2_compress_batch_jac(jac, n):
    return _compress_jac("blsmi_g2_compress_batch_jac", 288, 96, jac, n)


def decompress_batch_jac_dev(group, d_in, n, d_out_jac, d_out_inf, d_err, check_subgroup=True, stream=0):
    """device-pointer form (ints; d_out_inf may be 0): the records, flags and codes are in the caller's buffers when the call returns"""
    name = "blsmi_g1_decompress_batch_jac_dev" if group == "g1" else "blsmi_g2_decompress_batch_jac_dev"
    _check(_fn(name)(d_in or 0, int(check_subgroup), d_out_jac or 0, d_out_inf or 0, d_err or 0, n, stream or 0), name[len("blsmi_"):])


def compress_batch_jac_dev(group, d_pts_jac, n, d_out, stream=0):
    name = "blsmi_g1_compress_batch_jac_dev" if group == "g1" else "blsmi_g2_compress_batch_jac_dev"
    _check(_fn(name)(d_pts_jac or 0, d_out or 0, n, stream or 0), name[len("blsmi_"):])


# ---- committee aggregates, randomised (blsmi 0.16): many VerifyAggregateCommon under one pairing equation -----------------------------
_A_HEAD = [_u8p, _u64p, C.c_size_t, _u32p]                                 # msgs, msg_off, d, msg_idx
_A_HEAD_DOMAIN = [_u8p, _u8p, C.c_size_t, _u32p]                           # msgs32, domain, d, msg_idx
_A_TAIL = [_u64p, _u8p, _u8p, C.c_size_t, C.POINTER(C.c_int)]              # scalars, ok, ok_bitmap, m, combined
_A_HOST = [_u8p, C.c_size_t, _u32p, _u64p, _u8p] + _A_TAIL                 # pks, npk, idx, seg_off, sigs
_A_JAC = [_u64p, C.c_size_t, _u32p, _u64p, _u64p] + _A_TAIL
_A_DEV = [_V, _V, C.c_size_t, _V, _V, C.c_size_t, _V, _V, _V, _u64p, _V, C.c_size_t, C.POINTER(C.c_int), _V]
# the argument types of the ten entry points of 0.16, as include/blsmi.h declares them (tests/test_agg_common_rlc_cpu.py compares)
ARGTYPES_0_16 = {
    "blsmi_g2pubs_verify_aggregate_common_batch_rlc": _A_HEAD + _A_HOST,
    "blsmi_g1pubs_verify_aggregate_common_batch_rlc": _A_HEAD + _A_HOST,
    "blsmi_g1pubs_verify_aggregate_common_with_domain_batch_rlc": _A_HEAD_DOMAIN + _A_HOST,
    "blsmi_g2pubs_verify_aggregate_common_batch_rlc_jac": _A_HEAD + _A_JAC,
    "blsmi_g1pubs_verify_aggregate_common_batch_rlc_jac": _A_HEAD + _A_JAC,
    "blsmi_g1pubs_verify_aggregate_common_with_domain_batch_rlc_jac": _A_HEAD_DOMAIN + _A_JAC,
    "blsmi_g2pubs_verify_aggregate_common_batch_rlc_dev": _A_DEV,
    "blsmi_g1pubs_verify_aggregate_common_batch_rlc_dev": _A_DEV,
    "blsmi_g1pubs_verify_aggregate_common_with_domain_batch_rlc_dev": _A_DEV,
    "blsmi_debug_g2_sum_segmented_u64_pair": _SUM_U64,
}


def _agg_common_batch_rlc(name, kind, jac, msgs, msg_idx, pks, npk, idx, seg_off, sigs, scalars, domain8=None):
    """-> (ok, bitmap, combined); msgs: the table of d messages, msg_idx: one index into it per item, the registry and the committees as
    _agg_common_batch takes them"""
    so, pidx, _keep = _seg_args(idx, seg_off)
    m = so.size - 1
    ix, pix = _msg_idx(msg_idx, m)
    pkb, sgb = (192, 96) if kind == 0 else (96, 192)
    if domain8 is None:
        buf, off = _msgs(msgs)
        head = (_p8(buf), off.ctypes.data_as(_u64p))
    else:
        buf = _u8(b"".join(bytes(x) for x in msgs) or b"\0" * 32, 32 * max(len(msgs), 1))
        off = _u8(domain8, 8)
        head = (_p8(buf), _p8(off))
    if jac:
        p, pp = _j64(pks, pkb // 2 * 3 * npk)
        s, ps = _j64(sigs, sgb // 2 * 3 * m)
    else:
        p = _u8(pks, pkb * npk) if npk else np.zeros(1, np.uint8)
        s = _u8(sigs, sgb * m)
        pp, ps = _p8(p), _p8(s)
    r, pr = _scalars(scalars, m)
    ok = np.zeros(max(1, m), dtype=np.uint8)
    bitmap = np.zeros(max(1, (m + 7) // 8), dtype=np.uint8)
    comb = C.c_int(0)
    _check(_fn(name)(*head, len(msgs), pix, pp, npk, pidx, so.ctypes.data_as(_u64p), ps, pr, _p8(ok), _p8(bitmap), m, C.byref(comb)), name[len("blsmi_"):])
    return ok[:m].astype(bool), bitmap[:(m + 7) // 8].copy(), comb.value


def g2pubs_verify_aggregate_common_batch_rlc(msgs, msg_idx, pks, npk, idx, seg_off, sigs, scalars=None):
    """blsmi_g2pubs_verify_aggregate_common_batch_rlc -> (ok, bitmap, combined): item j is VerifyAggregateCommon(sigs[j], {pks[idx[k]] :
    seg_off[j] <= k < seg_off[j + 1]}, msgs[msg_idx[j]]); one pairing equation for all m (combined == 1) or, when it fails, the verdicts of
    g2pubs_verify_aggregate_common_batch (combined == 0).  scalars: m nonzero 64-bit integers, or None (the library draws them)."""
    return _agg_common_batch_rlc("blsmi_g2pubs_verify_aggregate_common_batch_rlc", 0, False, msgs, msg_idx, pks, npk, idx, seg_off, sigs, scalars)


def g1pubs_verify_aggregate_common_batch_rlc(msgs, msg_idx, pks, npk, idx, seg_off, sigs, scalars=None):
    return _agg_common_batch_rlc("blsmi_g1pubs_verify_aggregate_common_batch_rlc", 1, False, msgs, msg_idx, pks, npk, idx, seg_off, sigs, scalars)


def g1pubs_verify_aggregate_common_with_domain_batch_rlc(msgs32, domain8, msg_idx, pks, npk, idx, seg_off, sigs, scalars=None):
    return _agg_common_batch_rlc("blsmi_g1pubs_verify_aggregate_common_with_domain_batch_rlc", 2, False, msgs32, msg_idx, pks, npk, idx, seg_off, sigs, scalars, domain8)


def g2pubs_verify_aggregate_common_batch_rlc_jac(msgs, msg_idx, pks, npk, idx, seg_off, sigs, scalars=None):
    """the same over in-memory keys (288 bytes) and signatures (144 bytes)"""
    return _agg_common_batch_rlc("blsmi_g2pubs_verify_aggregate_common_batch_rlc_jac", 0, True, msgs, msg_idx, pks, npk, idx, seg_off, sigs, scalars)


def g1pubs_verify_aggregate_common_batch_rlc_jac(msgs, msg_idx, pks, npk, idx, seg_off, sigs, scalars=None):
    return _agg_common_batch_rlc("blsmi_g1pubs_verify_aggregate_common_batch_rlc_jac", 1, True, msgs, msg_idx, pks, npk, idx, seg_off, sigs, scalars)


def g1pubs_verify_aggregate_common_with_domain_batch_rlc_jac(msgs32, domain8, msg_idx, pks, npk, idx, seg_off, sigs, scalars=None):
    return _agg_common_batch_rlc("blsmi_g1pubs_verify_aggregate_common_with_domain_batch_rlc_jac", 2, True, msgs32, msg_idx, pks, npk, idx, seg_off, sigs, scalars, domain8)


def verify_aggregate_common_batch_rlc_dev(group, d_msgs, d_off_or_domain, d, d_msg_idx, d_pks, npk, d_idx, d_seg_off, d_sigs, d_ok, m, scalars=None, stream=0, domain=False):
    """device-pointer forms (ints): group "g2pubs" / "g1pubs" (domain=True: d_msgs holds d*32 bytes, d_off_or_domain the 8-byte domain); the m
    verdict bytes are in d_ok when the call returns; scalars stay on the host.  -> combined"""
    name = "blsmi_g2pubs_verify_aggregate_common_batch_rlc_dev" if group == "g2pubs" else \
        ("blsmi_g1pubs_verify_aggregate_common_with_domain_batch_rlc_dev" if domain else "blsmi_g1pubs_verify_aggregate_common_batch_rlc_dev")
    r, pr = _scalars(scalars, m)
    comb = C.c_int(0)
    _check(_fn(name)(d_msgs or 0, d_off_or_domain or 0, d, d_msg_idx or 0, d_pks or 0, npk, d_idx or 0, d_seg_off or 0, d_sigs or 0, pr, d_ok or 0, m,
                          C.byref(comb), stream or 0), name[len("blsmi_"):])
    return comb.value


def debug_g2_sum_segmented_u64_pair(pts, npk, scalars, idx, seg_off, in_inf=None):
    """g2_sum_segmented_u64 with pass 1 through the lane-pair ladder (k_g2_segsum_chunk_u64_pair), for the parity test"""
    return _sum_segmented_u64("blsmi_debug_g2_sum_segmented_u64_pair", 192, pts, npk, scalars, idx, seg_off, in_inf)


# ---- pairing products, randomised (blsmi 0.17): one equation for a batch of pairing products over a table of G2 points -------------
_P_TAIL = [C.c_size_t, _u64p, C.c_size_t, _u64p, _u8p, C.POINTER(C.c_int)]    # np, seg_off, m, scalars, is_one, combined
_P_DEV_TAIL = [C.c_size_t, _V, C.c_size_t, _u64p, _V, C.POINTER(C.c_int), _V]  # np, d_seg_off, m, scalars, d_is_one, combined, stream
# the argument types of the five entry points of 0.17, as include/blsmi.h declares them (tests/test_pprod_rlc_cpu.py compares)
ARGTYPES_0_17 = {
    "blsmi_pairing_product_batch_rlc": [_u8p, _u8p, _u8p, C.c_size_t, _u32p] + _P_TAIL,
    "blsmi_pairing_product_batch_rlc_jac": [_u64p, _u64p, C.c_size_t, _u32p] + _P_TAIL,
    "blsmi_pairing_product_batch_rlc_dev": [_V, _V, _V, C.c_size_t, _V] + _P_DEV_TAIL,
    "blsmi_pairing_product_batch_rlc_jac_dev": [_V, _V, C.c_size_t, _V] + _P_DEV_TAIL,
    "blsmi_debug_pairing_product_batch_rlc_dev_nosplit": [_V, _V, _V, C.c_size_t, _V] + _P_DEV_TAIL,
}


def _pprod_rlc(name, jac, g1, g2_tab, q_idx, seg_off, inf_flags, scalars, block=None):
    """block None: the forms of 0.17 -> (is_one, combined); an integer: the block-locating forms of 0.18 -> (is_one, combined, rechecked)"""
    pb, qb = (144, 288) if jac else (96, 192)
    a, t = _u8(g1), _u8(g2_tab)
    if a.size % pb or t.size % qb:
        raise ValueError("expected np*%d and nq*%d bytes, got %d and %d" % (pb, qb, a.size, t.size))
    n, nq = a.size // pb, t.size // qb
    so, m = _pprod_offsets(seg_off, n)
    if q_idx is None:
        if nq != n:
            raise ValueError("without q_idx the table has one entry per pair: %d entries, %d pairs" % (nq, n))
        ix, pix = None, None
    else:
        ix, pix = _msg_idx(q_idx, n)
        if n == 0:                                                         # (a table without pairs: the pointer still says "indexed")
            ix = np.zeros(1, dtype=np.uint32)
            pix = ix.ctypes.data_as(_u32p)
    r, pr = _scalars(scalars, m)
    one = np.zeros(max(1, m), dtype=np.uint8)
    comb, nre = C.c_int(0), C.c_size_t(0)
    fn = _fn(name)
    tail = (pr, _p8(one), C.byref(comb)) if block is None else (pr, block, _p8(one), C.byref(comb), C.byref(nre))
    if jac:
        (a, pa), (t, pt) = _j64(a, pb * n), _j64(t, qb * nq)
        rc = fn(pa, pt, nq, pix, n, so.ctypes.data_as(_u64p), m, *tail)
    else:
        f = _u8(inf_flags, n) if inf_flags is not None else None
        rc = fn(_p8(a), _p8(f), _p8(t), nq, pix, n, so.ctypes.data_as(_u64p), m, *tail)
    _check(rc, name[len("blsmi_"):])
    return (one[:m].copy(), comb.value) if block is None else (one[:m].copy(), comb.value, nre.value)


def _pprod_rlc_dev(name, points, nq, d_q_idx, np_, d_seg_off, m, d_is_one, scalars, stream, block=None):
    """the device-pointer forms; points: (d_g1, d_inf_flags, d_g2_tab) or, for in-memory points, (d_g1_jac, d_g2_tab_jac).  block None: the
    forms of 0.17 -> combined; the caller's `block`: those of 0.18 -> (combined, rechecked)"""
    r, pr = _scalars(scalars, m)
    comb, nre = C.c_int(0), C.c_size_t(0)
    out = (d_is_one or 0, C.byref(comb)) if block is None else (_block(block), d_is_one or 0, C.byref(comb), C.byref(nre))
    _check(_fn(name)(*(p or 0 for p in points), nq, d_q_idx or 0, np_, d_seg_off or 0, m, pr, *out, stream or 0), name[len("blsmi_"):])
    return comb.value if block is None else (comb.value, nre.value)


def pairing_product_batch_rlc(g1_aff, g2_tab, q_idx, seg_off, inf_flags=None, scalars=None):
    """blsmi_pairing_product_batch_rlc -> (is_one (m,) uint8, combined): pair k is (P_k, g2_tab[q_idx[k]]) (q_idx None: entry k), item j the
    pairs seg_off[j] <= k < seg_off[j + 1]; the verdicts of pairing_product_batch on the expanded table, from one randomised equation
    (combined == 1) or, when it fails, from the per-item path (combined == 0).  inf_flags[k] bit 0: P_k is the point at infinity.
    scalars: m nonzero 64-bit integers, or None (the library draws them)."""
    return _pprod_rlc("blsmi_pairing_product_batch_rlc", False, g1_aff, g2_tab, q_idx, seg_off, inf_flags, scalars)


def pairing_product_batch_rlc_jac(g1_jac, g2_tab_jac, q_idx, seg_off, scalars=None):
    """the same over in-memory points (144 / 288 bytes each, z == 0: infinity)"""
    return _pprod_rlc("blsmi_pairing_product_batch_rlc_jac", True, g1_jac, g2_tab_jac, q_idx, seg_off, None, scalars)


def pairing_product_batch_rlc_dev(d_g1, d_g2_tab, nq, d_q_idx, np_, d_seg_off, m, d_is_one, d_inf_flags=0, scalars=None, stream=0, nosplit=False):
    """device-pointer form (ints) over affine records; the m verdict bytes are in d_is_one when the call returns; scalars stay on the host.
    nosplit: blsmi_debug_pairing_product_batch_rlc_dev_nosplit (the measurement of the singleton by-pass).  -> combined"""
    name = "blsmi_debug_pairing_product_batch_rlc_dev_nosplit" if nosplit else "blsmi_pairing_product_batch_rlc_dev"
    return _pprod_rlc_dev(name, (d_g1, d_inf_flags, d_g2_tab), nq, d_q_idx, np_, d_seg_off, m, d_is_one, scalars, stream)


def pairing_product_batch_rlc_jac_dev(d_g1_jac, d_g2_tab_jac, nq, d_q_idx, np_, d_seg_off, m, d_is_one, scalars=None, stream=0):
    """device-pointer form over in-memory points (no flags: z == 0 is infinity) -> combined"""
    return _pprod_rlc_dev("blsmi_pairing_product_batch_rlc_jac_dev", (d_g1_jac, d_g2_tab_jac), nq, d_q_idx, np_, d_seg_off, m, d_is_one, scalars, stream)


# ---- pairing products, randomised, that find the bad items by blocks (blsmi 0.18) ---------------------------------------------------
_PL_TAIL = [C.c_size_t, _u64p, C.c_size_t, _u64p, C.c_size_t, _u8p, C.POINTER(C.c_int), C.POINTER(C.c_size_t)]        # np, seg_off, m, scalars, block, is_one, combined, rechecked
_PL_DEV_TAIL = [C.c_size_t, _V, C.c_size_t, _u64p, C.c_size_t, _V, C.POINTER(C.c_int), C.POINTER(C.c_size_t), _V]    # ..., d_is_one, combined, rechecked, stream
# the argument types of the four entry points of 0.18, as include/blsmi.h declares them (tests/test_pprod_rlc_locate_cpu.py compares)
ARGTYPES_0_18 = {
    "blsmi_pairing_product_batch_rlc_locate": [_u8p, _u8p, _u8p, C.c_size_t, _u32p] + _PL_TAIL,
    "blsmi_pairing_product_batch_rlc_locate_jac": [_u64p, _u64p, C.c_size_t, _u32p] + _PL_TAIL,
    "blsmi_pairing_product_batch_rlc_locate_dev": [_V, _V, _V, C.c_size_t, _V] + _PL_DEV_TAIL,
    "blsmi_pairing_product_batch_rlc_locate_jac_dev": [_V, _V, C.c_size_t, _V] + _PL_DEV_TAIL,
}


def _block(block):
    block = int(block)
    if block < 0:
        raise ValueError("block is 0 (automatic) or a number of items, got %d" % block)
    return block


def pairing_product_batch_rlc_locate(g1_aff, g2_tab, q_idx, seg_off, inf_flags=None, scalars=None, block=0):
    """blsmi_pairing_product_batch_rlc_locate -> (is_one (m,) uint8, combined, rechecked): pairing_product_batch_rlc with the items cut into
    blocks of `block` (0: automatic); when the one equation fails, only the items of the blocks whose own product is not one -- `rechecked`
    of them -- go through the per-item path, every other item's verdict is 1."""
    return _pprod_rlc("blsmi_pairing_product_batch_rlc_locate", False, g1_aff, g2_tab, q_idx, seg_off, inf_flags, scalars, _block(block))


def pairing_product_batch_rlc_locate_jac(g1_jac, g2_tab_jac, q_idx, seg_off, scalars=None, block=0):
    """the same over in-memory points (144 / 288 bytes each, z == 0: infinity)"""
    return _pprod_rlc("blsmi_pairing_product_batch_rlc_locate_jac", True, g1_jac, g2_tab_jac, q_idx, seg_off, None, scalars, _block(block))


def pairing_product_batch_rlc_locate_dev(d_g1, d_g2_tab, nq, d_q_idx, np_, d_seg_off, m, d_is_one, d_inf_flags=0, scalars=None, block=0, stream=0):
    """device-pointer form (ints) over affine records; the m verdict bytes are in d_is_one when the call returns; scalars stay on the host.
    -> (combined, rechecked)"""
    return _pprod_rlc_dev("blsmi_pairing_product_batch_rlc_locate_dev", (d_g1, d_inf_flags, d_g2_tab), nq, d_q_idx, np_, d_seg_off, m, d_is_one, scalars, stream, block)


def pairing_product_batch_rlc_locate_jac_dev(d_g1_jac, d_g2_tab_jac, nq, d_q_idx, np_, d_seg_off, m, d_is_one, scalars=None, block=0, stream=0):
    """device-pointer form over in-memory points (no flags: z == 0 is infinity) -> (combined, rechecked)"""
    return _pprod_rlc_dev("blsmi_pairing_product_batch_rlc_locate_jac_dev", (d_g1_jac, d_g2_tab_jac), nq, d_q_idx, np_, d_seg_off, m, d_is_one, scalars, stream, block)


# ---- scalar-field folds and Groth16 batches (blsmi 0.19) ------------------------------------------------------------------------------
_G16_TAIL = [_u8p, C.c_size_t, _u64p, C.c_size_t, _u8p, C.POINTER(C.c_int), C.POINTER(C.c_size_t)]                  # inputs, m, scalars, block, ok, combined, rechecked
_G16_DEV_TAIL = [_V, C.c_size_t, _u64p, C.c_size_t, _V, C.POINTER(C.c_int), C.POINTER(C.c_size_t), _V]              # d_inputs, m, scalars, block, d_ok, combined, rechecked, stream
# the argument types of the six entry points of 0.19, as include/blsmi.h declares them (tests/test_groth16_cpu.py compares)
ARGTYPES_0_19 = {
    "blsmi_fr_wsum_segmented_u64": [_u8p, C.c_size_t, _u64p, _u64p, C.c_size_t, _u8p],
    "blsmi_fr_wsum_segmented_u64_dev": [_V, C.c_size_t, _V, _V, C.c_size_t, _V, _V],
    "blsmi_groth16_verify_batch": [_u8p, _u8p, C.c_size_t, _u8p, _u8p] + _G16_TAIL,
    "blsmi_groth16_verify_batch_jac": [_u64p, _u64p, C.c_size_t, _u64p, _u64p] + _G16_TAIL,
    "blsmi_groth16_verify_batch_dev": [_V, _V, C.c_size_t, _V, _V] + _G16_DEV_TAIL,
    "blsmi_groth16_verify_batch_jac_dev": [_V, _V, C.c_size_t, _V, _V] + _G16_DEV_TAIL,
}


def fr_wsum_segmented_u64(vals, ncol, weights, seg_off):
    """blsmi_fr_wsum_segmented_u64 -> (nseg, ncol + 1, 32) uint8: per segment of rows the sum of its 64-bit weights and, per column, the
    weighted sum of its scalars mod r, every output fully reduced.  vals: n * ncol scalars of 32 big-endian bytes, row-major (any 256-bit
    value); weights: n integers below 2^64; seg_off: nseg + 1 offsets from 0 to n."""
    ncol = int(ncol)
    if ncol < 0:
        raise ValueError("ncol is a number of columns, got %d" % ncol)
    so = np.ascontiguousarray(np.asarray(seg_off, dtype=np.uint64))
    if so.ndim != 1 or so.size < 1 or int(so[0]) != 0 or np.any(so[1:] < so[:-1]):
        raise ValueError("seg_off: nseg + 1 offsets from 0, non-decreasing")
    nseg, n = so.size - 1, int(so[-1])
    v = _u8(vals, 32 * ncol * n)
    w = np.ascontiguousarray(np.asarray([int(x) for x in weights], dtype=np.uint64))
    if w.shape != (n,):
        raise ValueError("need one weight per row: %d rows, %d weights" % (n, w.size))
    out = np.zeros((nseg, ncol + 1, 32), dtype=np.uint8)
    _check(_fn("blsmi_fr_wsum_segmented_u64")(_p8(v), ncol, w.ctypes.data_as(_u64p) if n else None, so.ctypes.data_as(_u64p), nseg, _p8(out.reshape(-1))),
           "fr_wsum_segmented_u64")
    return out


def fr_wsum_segmented_u64_dev(d_vals, ncol, d_weights, d_seg_off, nseg, d_out, stream=0):
    """device-pointer form (ints); the nseg * (ncol + 1) scalars are in d_out when the call returns"""
    _check(_fn("blsmi_fr_wsum_segmented_u64_dev")(d_vals or 0, ncol, d_weights or 0, d_seg_off or 0, nseg, d_out or 0, stream or 0), "fr_wsum_segmented_u64_dev")


def _groth16(name, jac, vk_g1, vk_g2, proof_g1, proof_g2, inputs, nin, scalars, block):
    pb, qb = (144, 288) if jac else (96, 192)
    nin = int(nin)
    if nin < 0:
        raise ValueError("nin is a number of public inputs, got %d" % nin)
    k1, k2 = _u8(vk_g1, pb * (nin + 2)), _u8(vk_g2, qb * 3)
    a, b = _u8(proof_g1), _u8(proof_g2)
    if b.size % qb or a.size != 2 * pb * (b.size // qb):
        raise ValueError("expected m*%d bytes of B_j and 2*m*%d bytes of A_j, C_j, got %d and %d" % (qb, pb, b.size, a.size))
    m = b.size // qb
    x = _u8(inputs if inputs is not None else b"", 32 * nin * m)
    r, pr = _scalars(scalars, m)
    block = _block(block)
    ok = np.zeros(max(1, m), dtype=np.uint8)
    comb, nre = C.c_int(0), C.c_size_t(0)
    fn = _fn(name)
    if jac:
        (k1, pk1), (k2, pk2), (a, pa), (b, pb_) = _j64(k1, k1.size), _j64(k2, k2.size), _j64(a, a.size), _j64(b, b.size)
    else:
        pk1, pk2, pa, pb_ = _p8(k1), _p8(k2), _p8(a), _p8(b)
    _check(fn(pk1, pk2, nin, pa, pb_, _p8(x), m, pr, block, _p8(ok), C.byref(comb), C.byref(nre)), name[len("blsmi_"):])
    return ok[:m].copy(), comb.value, nre.value


def groth16_verify_batch(vk_g1, vk_g2, proof_g1, proof_g2, inputs, nin, scalars=None, block=0):
    """blsmi_groth16_verify_batch -> (ok (m,) uint8, combined, rechecked): m Groth16 proofs of one circuit with nin public inputs.  vk_g1:
    alpha, IC_0 .. IC_nin (96 bytes each); vk_g2: beta, gamma, delta (192 each); proof_g1: A_j, C_j interleaved; proof_g2: B_j; inputs: m * nin
    scalars of 32 big-endian bytes, item-major (None when nin == 0).  ok[j] is the verdict of pairing_product_batch on (A_j, B_j),
    (-alpha, beta), (-L_j, gamma), (-C_j, delta); scalars and block as pairing_product_batch_rlc_locate."""
    return _groth16("blsmi_groth16_verify_batch", False, vk_g1, vk_g2, proof_g1, proof_g2, inputs, nin, scalars, block)


def groth16_verify_batch_jac(vk_g1_jac, vk_g2_jac, proof_g1_jac, proof_g2_jac, inputs, nin, scalars=None, block=0):
    """the same over in-memory points (144 / 288 bytes each, z == 0: infinity)"""
    return _groth16("blsmi_groth16_verify_batch_jac", True, vk_g1_jac, vk_g2_jac, proof_g1_jac, proof_g2_jac, inputs, nin, scalars, block)


def _groth16_dev(name, d_vk_g1, d_vk_g2, nin, d_proof_g1, d_proof_g2, d_inputs, m, d_ok, scalars, block, stream):
    r, pr = _scalars(scalars, m)
    comb, nre = C.c_int(0), C.c_size_t(0)
    _check(_fn(name)(d_vk_g1 or 0, d_vk_g2 or 0, nin, d_proof_g1 or 0, d_proof_g2 or 0, d_inputs or 0, m, pr, _block(block), d_ok or 0, C.byref(comb), C.byref(nre), stream or 0),
           name[len("blsmi_"):])
    return comb.value, nre.value


def groth16_verify_batch_dev(d_vk_g1, d_vk_g2, nin, d_proof_g1, d_proof_g2, d_inputs, m, d_ok, scalars=None, block=0, stream=0):
    """device-pointer form (ints) over affine records; the m verdict bytes are in d_ok when the call returns; scalars stay on the host.
    -> (combined, rechecked)"""
    return _groth16_dev("blsmi_groth16_verify_batch_dev", d_vk_g1, d_vk_g2, nin, d_proof_g1, d_proof_g2, d_inputs, m, d_ok, scalars, block, stream)


def groth16_verify_batch_jac_dev(d_vk_g1_jac, d_vk_g2_jac, nin, d_proof_g1_jac, d_proof_g2_jac, d_inputs, m, d_ok, scalars=None, block=0, stream=0):
    """device-pointer form over in-memory points -> (combined, rechecked)"""
    return _groth16_dev("blsmi_groth16_verify_batch_jac_dev", d_vk_g1_jac, d_vk_g2_jac, nin, d_proof_g1_jac, d_proof_g2_jac, d_inputs, m, d_ok, scalars, block, stream)
