"""Thin ctypes layer over the C ABI of libblsmi.so (include/blsmi.h).  Host code only: every
computation happens in the HIP kernels; a missing library or device raises, nothing falls back."""
import ctypes as C

import numpy as np

from . import _native

_u8p = C.POINTER(C.c_uint8)
_u32p = C.POINTER(C.c_uint32)
_u64p = C.POINTER(C.c_uint64)


class BlsmiError(RuntimeError):
    pass


_ERR = {-1: "no usable HIP device", -2: "HIP runtime call failed", -3: "bad argument", -4: "out of memory", -5: "RCCL unavailable or collective failed", -6: "OS random source failed"}


def _check(rc, what):
    if rc != 0:
        raise BlsmiError("%s failed: %s (%d)" % (what, _ERR.get(rc, "unknown"), rc))


def _lib():
    return _native.load()


_bound = {}


def _fn(name):
    """The entry point `name` with the return and argument types include/blsmi.h declares for it (_native.signatures()), so that a call passes
    plain values: Python ints for size_t, int and void * parameters (0 or None: a null pointer), numpy pointers for typed pointers, byref()
    for out-parameters.  A private function object, bound once: the attributes of the library _lib() returns stay untyped for their other
    users.  Two threads that meet here first bind one object each and keep the same one."""
    fn = _bound.get(name)
    if fn is None:
        fn = _lib()[name]
        restype, argtypes = _native.signatures()[name]
        fn.restype = restype
        fn.argtypes = argtypes
        fn = _bound.setdefault(name, fn)
    return fn


def _call(name, *args):
    rc = (_bound.get(name) or _fn(name))(*args)
    if rc != 0:
        _check(rc, name)


def _u8(x, nbytes=None):
    a = np.frombuffer(x, dtype=np.uint8) if isinstance(x, (bytes, bytearray, memoryview)) else np.ascontiguousarray(x, dtype=np.uint8).reshape(-1)
    if nbytes is not None and a.size != nbytes:
        raise ValueError("expected %d bytes, got %d" % (nbytes, a.size))
    return a


def _ptr(a, ptype):
    """a typed pointer to the data of a numpy array that keeps the array alive: what a.ctypes.data_as(ptype) gives, at half its cost (no
    ctypes view of the array is built on the way)"""
    p = C.cast(a.__array_interface__["data"][0], ptype)
    p._arr = a
    return p


def _p8(a):
    return _ptr(a, _u8p) if a is not None and a.size else None


def _p32(a):
    return _ptr(a, _u32p)


def _p64(a):
    return _ptr(a, _u64p)


def _flags(flags, n):
    """optional per-element bytes (infinity flags): NULL without them"""
    return _p8(_u8(flags, n)) if flags is not None else None


def _pubs(group):
    return "g2pubs" if group == "g2pubs" else "g1pubs"


def _g12(group):
    return "g1" if group == "g1" else "g2"


def init(device=0):
    """Bind this process to one device (one rank per GPU under torchrun)."""
    _call("blsmi_init", int(device))


def init_devices(ndev=0):
    """Drive the first ndev devices (0 = all visible) from this one process: large verify / pairing batches are split
    over them inside the library (RCCL bitmap all-reduce / partial-product all-gather), see include/blsmi.h."""
    _call("blsmi_init_devices", int(ndev))


def debug_alias_own(ptr, nbytes, device_index):
    """TEST HOOK (BLSMI_DEVICE_ALIAS): the device-pointer range belongs to logical device `device_index` (include/blsmi.h)."""
    _call("blsmi_debug_alias_own", int(ptr), int(nbytes), int(device_index))


def trim(keep_bytes_per_context=0):
    """Give the temporaries idle call contexts hold beyond keep_bytes_per_context (and the pool cache) back to the driver; bytes freed."""
    freed = C.c_size_t(0)
    _call("blsmi_trim", int(keep_bytes_per_context), C.byref(freed))
    return int(freed.value)


def held_bytes():
    """device memory the call contexts currently hold for temporaries (all devices)"""
    return int(_fn("blsmi_held_bytes")())


SHAPE_PAIRING, SHAPE_MILLER_LOOP, SHAPE_FINAL_EXP, SHAPE_G2_PREPARE, SHAPE_VERIFY, SHAPE_SIGN, SHAPE_VERIFY_DOMAIN, SHAPE_POINT_ADD = range(8)


def prefer_cpu(shape, n):
    """True when n operations of `shape` in one call finish sooner on one core of the upstream CPU path (include/blsmi.h)"""
    return bool(_fn("blsmi_prefer_cpu")(int(shape), int(n)))


def device_leases(device_index):
    """context leases device `device_index` has served since initialisation (-1: no such device)"""
    return int(_fn("blsmi_debug_device_leases")(int(device_index)))


def device_count():
    return int(_fn("blsmi_device_count")())


def shard_count():
    return int(_fn("blsmi_shard_count")())


def set_latency_threshold(max_tuples):
    """Batches of at most max_tuples tuples take the latency path (one tuple per wave); 0 = always the lane-pair kernels."""
    _call("blsmi_set_latency_threshold", int(max_tuples))


def set_quad_threshold(max_tuples):
    """Batches above the latency threshold and of at most max_tuples tuples take the lane-quad kernels (four lanes per tuple); 0 = off."""
    _call("blsmi_set_quad_threshold", int(max_tuples))


def set_row_threshold(min_tuples, max_tuples):
    """A lone pairing / verify call of min_tuples .. max_tuples tuples takes the lane-row kernels (sixteen lanes per tuple); max 0 = off."""
    _call("blsmi_set_row_threshold", int(min_tuples), int(max_tuples))


ROW_DEFAULT = (2048, 8192)


def set_option(name, value):
    """run-time switch between code paths with identical results: "agg_cofactor_pow", "msm_sort", "dup_force_sort" (include/blsmi.h)"""
    _check(_fn("blsmi_set_option")(name.encode(), int(value)), "blsmi_set_option(%s)" % name)


def set_mul_assume_subgroup(on=True):
    """scalar multiplications through the curve endomorphisms (multiplicands in the prime-order subgroup; the default) or,
    with on=False, the plain windowed ladder that serves every curve point"""
    _call("blsmi_set_mul_assume_subgroup", 1 if on else 0)


def shutdown():
    _fn("blsmi_shutdown")()


def version():
    return _fn("blsmi_version")().decode()


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


# ---- what the entry points have in common: the message head (offsets or domain) and the records (wire bytes or in-memory words) --------
def _msg_head(msgs):
    """the messages as the two leading arguments: concatenated bytes, n + 1 offsets"""
    buf, off = _msgs(msgs)
    return _p8(buf), _p64(off)


def _domain_head(msgs32, domain8, empty=0):
    """the *_with_domain forms' two leading arguments: n x 32 message bytes, the 8-byte domain.  empty: the placeholder bytes that stand in for
    no message at all (0: NULL)"""
    n = len(msgs32)
    buf = _u8(b"".join(bytes(m) for m in msgs32), 32 * n) if n or not empty else np.zeros(empty, np.uint8)
    return _p8(buf), _p8(_u8(domain8, 8))


def _one_msg(msg):
    """the *_aggregate_common forms' two leading arguments: the message (a placeholder byte for the empty one), its length"""
    return _p8(_u8(bytes(msg) or b"\0")), len(msg)


def _recs(x, nbytes, jac=False, pad=False):
    """nbytes of records: wire bytes as uint8_t * (NULL when there are none or, with pad, a placeholder byte), or in-memory points as
    uint64_t * (a placeholder word when there are none); the size is checked unless a placeholder stands in"""
    if nbytes or not (jac or pad):
        a = _u8(x, nbytes)
        if not a.size:
            return None
    else:
        a = np.zeros(8 if jac else 1, np.uint8)
    return _ptr(a, _u64p if jac else _u8p)


def _sizes(kind, jac=False):
    """(key bytes, signature bytes): kind 0 g2pubs, otherwise g1pubs; an in-memory point is half as large again as its affine record"""
    pkb, sgb = (192, 96) if kind == 0 else (96, 192)
    return (pkb // 2 * 3, sgb // 2 * 3) if jac else (pkb, sgb)


# ---- pairing ---------------------------------------------------------------------------------------
class HostBuffer:
    """Page-locked host memory from the library (blsmi_host_alloc) as a numpy uint8 array: `.a`.  Arrays handed to the host entry
    points from such memory are copied by DMA instead of being staged.  The block is returned to the runtime when the LAST numpy view of
    it is gone: `.a` and every slice taken from it keep the allocation alive (they hold the ctypes block whose finaliser frees it), so
    .free() -- or dropping the HostBuffer -- can never pull memory from under a view that is still in use."""

    def __init__(self, nbytes):
        import weakref
        p = C.c_void_p()
        _call("blsmi_host_alloc", int(nbytes), C.byref(p))
        self.nbytes = int(nbytes)
        if nbytes:
            block = (C.c_uint8 * self.nbytes).from_address(p.value)         # every numpy view below references this object
            self._finalizer = weakref.finalize(block, _fn("blsmi_host_free"), p.value)
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


def _pairs(name, g1_aff, g2_aff, n, out=None):
    if out is None:
        out = np.zeros((n, 72), dtype=np.uint64)
    _call(name, _recs(g1_aff, 96 * n), _recs(g2_aff, 192 * n), _p64(out), n)
    return out


def pairing_batch(g1_aff, g2_aff, n, out=None):
    """n x 96 B G1 affine, n x 192 B G2 affine -> (n, 72) uint64: the reference's in-memory FQ12."""
    return _pairs("blsmi_pairing_batch", g1_aff, g2_aff, n, out)


def miller_loop_batch(g1_aff, g2_aff, n):
    return _pairs("blsmi_miller_loop_batch", g1_aff, g2_aff, n)


def final_exponentiation_batch(fq12):
    x = np.ascontiguousarray(fq12, dtype=np.uint64).reshape(-1, 72)
    out = np.zeros_like(x)
    _call("blsmi_final_exponentiation_batch", _p64(x), _p64(out), x.shape[0])
    return out


def pairing_batch_dev(d_g1, d_g2, d_out, n, stream=0):
    """Device-pointer form (ints, e.g. torch.Tensor.data_ptr()); enqueues and synchronises `stream`."""
    _call("blsmi_pairing_batch_dev", d_g1, d_g2, d_out, n, stream)


def verify_batch_dev(group, d_msgs, d_off, d_pks, d_sigs, d_inf, d_ok, n, stream=0):
    _call("blsmi_%s_verify_batch_dev" % _pubs(group), d_msgs, d_off, d_pks, d_sigs, d_inf, d_ok, n, stream)


def g1pubs_verify_with_domain_batch_dev(d_msgs32, d_domain, d_pks, d_sigs, d_inf, d_ok, n, stream=0):
    """VerifyWithDomain (g1pubs/bls.go:171-174) with everything resident on the device (ints = device pointers)"""
    _call("blsmi_g1pubs_verify_with_domain_batch_dev", d_msgs32, d_domain, d_pks, d_sigs, d_inf, d_ok, n, stream)


def mul_batch_dev(group, d_pts, d_scalars, d_out, d_out_inf, n, stream=0, any_point=False):
    """k_i * P_i with everything resident on the device (ints = device pointers; d_pts = 0: the group generator).
    any_point: multiplicands outside the prime-order subgroup are allowed for this call (see g1_mul_batch)."""
    if any_point:
        _call("blsmi_%s_mul_batch_dev_ex" % _g12(group), d_pts, d_scalars, d_out, d_out_inf, n, stream, MUL_ANY_POINT)
    else:
        _call("blsmi_%s_mul_batch_dev" % _g12(group), d_pts, d_scalars, d_out, d_out_inf, n, stream)


def sum_dev(group, d_pts, d_in_inf, n, d_out, stream=0):
    """sum of n resident points -> affine bytes at d_out (device); returns True when the sum is the point at infinity."""
    oinf = C.c_int(0)
    _call("blsmi_%s_sum_dev" % _g12(group), d_pts, d_in_inf, n, d_out, C.byref(oinf), stream)
    return bool(oinf.value)


def msm_dev(group, d_pts, d_scalars, n, d_out, stream=0, any_point=False):
    """sum_i k_i P_i over resident points and scalars -> affine bytes at d_out (device); True when it is the point at infinity."""
    oinf = C.c_int(0)
    if any_point:
        _call("blsmi_%s_msm_dev_ex" % _g12(group), d_pts, d_scalars, n, d_out, C.byref(oinf), stream, MUL_ANY_POINT)
    else:
        _call("blsmi_%s_msm_dev" % _g12(group), d_pts, d_scalars, n, d_out, C.byref(oinf), stream)
    return bool(oinf.value)


def verify_aggregate_common_dev(group, d_pks, n, msg, sig, domain=None, stream=0):
    """VerifyAggregateCommon (g2pubs/bls.go:275-278, g1pubs/bls.go:287-297) with the n public keys resident on the device (int =
    device pointer); msg / sig = host bytes; domain (8 bytes, g1pubs only): the *WithDomain form over a 32-byte message."""
    ok = C.c_int(0)
    if domain is not None:
        assert group == "g1pubs"
        _call("blsmi_g1pubs_verify_aggregate_common_with_domain_dev", d_pks, n, _p8(_u8(msg, 32)), _p8(_u8(domain, 8)), _p8(_u8(sig, 192)), C.byref(ok), stream)
    else:
        _call("blsmi_%s_verify_aggregate_common_dev" % _pubs(group), d_pks, n, _p8(_u8(msg)), len(msg), _p8(_u8(sig, 96 if group == "g2pubs" else 192)), C.byref(ok), stream)
    return bool(ok.value)


def verify_aggregate_dev(group, d_msgs, d_off, d_pks, sig, n, stream=0):
    """VerifyAggregate with messages / offsets / keys resident on the device; sig = host bytes of the aggregate signature."""
    ok = C.c_int(0)
    _call("blsmi_%s_verify_aggregate_dev" % _pubs(group), d_msgs, d_off, d_pks, _p8(_u8(sig, 96 if group == "g2pubs" else 192)), n, C.byref(ok), stream)
    return bool(ok.value)


def verify_aggregate_with_domain_dev(d_msgs32, d_domain, d_pks, sig, n, stream=0):
    ok = C.c_int(0)
    _call("blsmi_g1pubs_verify_aggregate_with_domain_dev", d_msgs32, d_domain, d_pks, _p8(_u8(sig, 192)), n, C.byref(ok), stream)
    return bool(ok.value)


# ---- prepared public keys (g2pubs): G2AffineToPrepared once, Miller loops that read the lines (blsmi 0.4) ----
G2_PREPARED_BYTES = 24704


def g2_prepare_batch_dev(d_g2_aff, n, d_prepared, stream=0):
    """n resident G2 points -> n tables of G2_PREPARED_BYTES at d_prepared (device)."""
    _call("blsmi_g2_prepare_batch_dev", d_g2_aff, n, d_prepared, stream)


def g2_prepared_export_dev(d_prepared, n, d_out, stream=0):
    """the reference's G2Prepared.coeffs of n tables: n x 68 x 3 x 12 uint64 at d_out (device)."""
    _call("blsmi_g2_prepared_export_dev", d_prepared, n, d_out, stream)


def g2_prepare_batch(g2_aff, n):
    """G2AffineToPrepared (g2.go:639-801) of n host points: (n, 68, 3, 12) uint64 -- coefficient triples of FQ2 as c0 | c1 limbs."""
    out = np.empty((n, 68, 3, 12), dtype=np.uint64)
    _call("blsmi_g2_prepare_batch", _recs(g2_aff, 192 * n), n, _p64(out))
    return out


class PreparedKeys:
    """n g2pubs public keys prepared into tables the library owns (blsmi_g2_prepared_create); .ptr is the device pointer."""

    def __init__(self, g2_aff, n):
        self._create("blsmi_g2_prepared_create", _recs(g2_aff, 192 * n), n)

    def _create(self, name, pts, n):
        h = C.c_void_p(0)
        _call(name, pts, n, C.byref(h))
        self.ptr, self.n = h.value, n

    def close(self):
        if self.ptr:
            _call("blsmi_g2_prepared_destroy", self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _prepared(prepared, key_idx):
    """the prepared forms' two arguments after the messages: the tables (a PreparedKeys or a device pointer), the optional key indices"""
    return prepared.ptr if isinstance(prepared, PreparedKeys) else prepared, None if key_idx is None else _p32(np.ascontiguousarray(key_idx, dtype=np.uint32))


def g2pubs_verify_batch_prepared(msgs, prepared, key_idx, sigs, inf_flags=None):
    """g2pubs.Verify x n, host buffers, keys prepared (a PreparedKeys or a device pointer): (ok bool array, packed bitmap)."""
    n = len(msgs)
    ok = np.empty(n, dtype=np.uint8)
    bm = np.empty((n + 7) // 8, dtype=np.uint8)
    _call("blsmi_g2pubs_verify_batch_prepared", *_msg_head(msgs), *_prepared(prepared, key_idx), _recs(sigs, 96 * n), _flags(inf_flags, n), _p8(ok), _p8(bm), n)
    return ok.astype(bool), bm


def pairing_batch_prepared_dev(d_g1, d_prepared, d_key_idx, d_out, n, stream=0):
    _call("blsmi_pairing_batch_prepared_dev", d_g1, d_prepared, d_key_idx, d_out, n, stream)


def g2pubs_verify_batch_prepared_dev(d_msgs, d_off, d_prepared, d_key_idx, d_sigs, d_inf, d_ok, n, stream=0):
    _call("blsmi_g2pubs_verify_batch_prepared_dev", d_msgs, d_off, d_prepared, d_key_idx, d_sigs, d_inf, d_ok, n, stream)


def _verify_aggregate_prepared(name, jac, msgs, prepared, key_idx, sig):
    ok = C.c_int(0)
    _call(name, *_msg_head(msgs), *_prepared(prepared, key_idx), _recs(sig, 144 if jac else 96, jac), len(msgs), C.byref(ok))
    return bool(ok.value)


def g2pubs_verify_aggregate_prepared(msgs, prepared, key_idx, sig):
    """Signature.VerifyAggregate over prepared keys, host buffers (a PreparedKeys or a device pointer)."""
    return _verify_aggregate_prepared("blsmi_g2pubs_verify_aggregate_prepared", False, msgs, prepared, key_idx, sig)


def g2pubs_verify_aggregate_prepared_dev(d_msgs, d_off, d_prepared, d_key_idx, sig, n, stream=0):
    ok = C.c_int(0)
    _call("blsmi_g2pubs_verify_aggregate_prepared_dev", d_msgs, d_off, d_prepared, d_key_idx, _p8(_u8(sig, 96)), n, C.byref(ok), stream)
    return bool(ok.value)


# ---- groups ----------------------------------------------------------------------------------------
MUL_ANY_POINT = 1          # BLSMI_MUL_ANY_POINT (include/blsmi.h)


def _ex(name, any_point):
    """(the symbol, its trailing arguments): the *_ex form with BLSMI_MUL_ANY_POINT for any_point"""
    return (name + "_ex", (MUL_ANY_POINT,)) if any_point else (name, ())


def _mul(name, pb, pts, scalars, n, any_point):
    name, flags = _ex(name, any_point)
    out = np.empty(pb * n, dtype=np.uint8)              # every byte is written by the call
    inf = np.empty(n, dtype=np.uint8)
    _call(name, _recs(pts, pb * n), _recs(scalars, 32 * n), _p8(out), _p8(inf), n, *flags)
    return out.reshape(n, pb), inf.astype(bool)


def g1_mul_batch(pts, scalars, n, any_point=False):
    """k_i * P_i (G1Affine.MulFR, g1.go:80-90).  The default ladder runs through the curve endomorphism and REQUIRES multiplicands
    in the prime-order subgroup (hash points, generators, keys / signatures that passed Deserialize's subgroup check): an on-curve
    point outside it gives a different point, silently.  any_point=True selects, for this call only, the plain windowed ladder
    that serves every curve point like the reference does (e.g. after g1_decompress_batch(check_subgroup=False))."""
    return _mul("blsmi_g1_mul_batch", 96, pts, scalars, n, any_point)


def g2_mul_batch(pts, scalars, n, any_point=False):
    """k_i * P_i (G2Affine.MulFR, g2.go:92-102); subgroup points unless any_point=True -- see g1_mul_batch."""
    return _mul("blsmi_g2_mul_batch", 192, pts, scalars, n, any_point)


def _mul_hashed(name, jac, rec, head, n, sks):
    """sk_i * (the point `head` names: the hash of message i or, without a head, the generator) -> n records of rec bytes: wire bytes and
    infinity flags, or in-memory points"""
    k = _recs(sks, 32 * n)
    if jac:
        out = np.zeros(max(1, rec // 8 * n), dtype=np.uint64)
        _call(name, *head, k, _p64(out), n)
        return out[:rec // 8 * n].view(np.uint8).reshape(n, rec)
    out = np.zeros((n, rec), dtype=np.uint8); inf = np.zeros(n, dtype=np.uint8)
    _call(name, *head, k, _p8(out.reshape(-1)), _p8(inf), n)
    return out, inf


def g1_mul_generator_batch(scalars, n):
    """k_i * G1 generator (PrivToPub of g1pubs)."""
    out, inf = _mul_hashed("blsmi_g1_mul_generator_batch", False, 96, (), n, scalars)
    return out, inf.astype(bool)


def g2_mul_generator_batch(scalars, n):
    """k_i * G2 generator (PrivToPub of g2pubs)."""
    out, inf = _mul_hashed("blsmi_g2_mul_generator_batch", False, 192, (), n, scalars)
    return out, inf.astype(bool)


def _msm(name, pb, pts, scalars, n, any_point):
    name, flags = _ex(name, any_point)
    out = np.zeros(pb, dtype=np.uint8)
    oinf = C.c_int(0)
    _call(name, _recs(pts, pb * n, pad=True), _recs(scalars, 32 * n, pad=True), n, _p8(out), C.byref(oinf), *flags)
    return None if oinf.value else out.tobytes()


def g1_msm(pts, scalars, n, any_point=False):
    """sum_i k_i * P_i -> 96 affine bytes, or None for the point at infinity (subgroup points unless any_point=True, see g1_mul_batch)."""
    return _msm("blsmi_g1_msm", 96, pts, scalars, n, any_point)


def g2_msm(pts, scalars, n, any_point=False):
    return _msm("blsmi_g2_msm", 192, pts, scalars, n, any_point)


def _sum(name, pb, pts, n, in_inf):
    out = np.zeros(pb, dtype=np.uint8)
    oinf = C.c_int(0)
    _call(name, _recs(pts, pb * n, pad=True), _flags(in_inf, n), n, _p8(out), C.byref(oinf))
    return (None if oinf.value else out.tobytes())


def g1_sum(pts, n, in_inf=None):
    """Sum of n affine points -> 96 bytes, or None for the point at infinity."""
    return _sum("blsmi_g1_sum", 96, pts, n, in_inf)


def g2_sum(pts, n, in_inf=None):
    return _sum("blsmi_g2_sum", 192, pts, n, in_inf)


# ---- hash to curve ---------------------------------------------------------------------------------
def _hash(name, ob, head, n):
    out = np.zeros((n, ob), dtype=np.uint8)
    _call(name, *head, _p8(out.reshape(-1)), n)
    return out


def hash_g1_batch(msgs):
    return _hash("blsmi_hash_g1_batch", 96, _msg_head(msgs), len(msgs))


def hash_g2_batch(msgs):
    return _hash("blsmi_hash_g2_batch", 192, _msg_head(msgs), len(msgs))


def hash_g2_with_domain_batch(msgs32, domain8):
    return _hash("blsmi_hash_g2_with_domain_batch", 192, _domain_head(msgs32, domain8), len(msgs32))


# ---- sign: sk_i * H(m_i) in one call (the hash points stay on the device) ---------------------------
def g2pubs_sign_batch(msgs, sks):
    """blsmi_g2pubs_sign_batch: n x 96-byte signatures sk_i * HashG1(m_i) (g2pubs/bls.go:132-135) and their infinity flags"""
    return _mul_hashed("blsmi_g2pubs_sign_batch", False, 96, _msg_head(msgs), len(msgs), sks)


def g1pubs_sign_batch(msgs, sks):
    """blsmi_g1pubs_sign_batch: n x 192-byte signatures sk_i * HashG2(m_i) (g1pubs/bls.go:132-135)"""
    return _mul_hashed("blsmi_g1pubs_sign_batch", False, 192, _msg_head(msgs), len(msgs), sks)


def g1pubs_sign_with_domain_batch(msgs32, domain8, sks):
    """blsmi_g1pubs_sign_with_domain_batch: sk_i * HashG2WithDomain(m_i, domain) (g1pubs/bls.go:138-141)"""
    return _mul_hashed("blsmi_g1pubs_sign_with_domain_batch", False, 192, _domain_head(msgs32, domain8), len(msgs32), sks)


# ---- verify ----------------------------------------------------------------------------------------
def _scalars(scalars, n):
    """caller scalars (n nonzero 64-bit integers) as a pointer, or None: the library draws fresh ones"""
    if scalars is None:
        return None
    r = np.ascontiguousarray(np.asarray([int(x) for x in scalars], dtype=np.uint64))
    if r.shape != (n,):
        raise ValueError("need one scalar per tuple")
    return _p64(r)


def _block(block):
    block = int(block)
    if block < 0:
        raise ValueError("block is 0 (automatic) or a number of items, got %d" % block)
    return block


def _msg_idx(msg_idx, n):
    ix = np.ascontiguousarray(np.asarray(msg_idx, dtype=np.uint32))
    if ix.shape != (n,):
        raise ValueError("need one message index per tuple")
    return _p32(ix) if n else None


def _grouped_head(msgs, msg_idx, n, domain8=None):
    """the grouped forms' four leading arguments: the table of d messages (or d x 32 bytes and the domain), d, n indices into the table"""
    pix = _msg_idx(msg_idx, n)
    return (_msg_head(msgs) if domain8 is None else _domain_head(msgs, domain8, 32)) + (len(msgs), pix)


def _verify(name, kind, jac, head, n, pks, sigs, inf_flags=None, rlc=False, scalars=None, block=None, bitmap=True):
    """n Verify()s through any of the batch entry points -> (ok, bitmap[, combined][, rechecked]).  head: the leading arguments (_msg_head,
    _domain_head or _grouped_head); jac: keys and signatures are in-memory points (no infinity flags); rlc: a randomised form (scalars in,
    combined out); block: a block-locating form (block in, rechecked out); bitmap=False: the entry point gets NULL for its bitmap."""
    pkb, sgb = _sizes(kind, jac)
    args = head + (_recs(pks, pkb * n, jac), _recs(sigs, sgb * n, jac)) + (() if jac else (_flags(inf_flags, n),))
    ok = np.zeros(n, dtype=np.uint8)
    bm = np.zeros((n + 7) // 8, dtype=np.uint8)
    comb, nre = C.c_int(0), C.c_size_t(0)
    if rlc:
        args += (_scalars(scalars, n),)
    if block is not None:
        args += (_block(block),)
    args += (_p8(ok), _p8(bm) if bitmap else None, n) + ((C.byref(comb),) if rlc else ()) + ((C.byref(nre),) if block is not None else ())
    _call(name, *args)
    return (ok.astype(bool), bm) + ((comb.value,) if rlc else ()) + ((nre.value,) if block is not None else ())


def g2pubs_verify_batch(msgs, pks, sigs, inf_flags=None):
    return _verify("blsmi_g2pubs_verify_batch", 0, False, _msg_head(msgs), len(msgs), pks, sigs, inf_flags)


def g1pubs_verify_batch(msgs, pks, sigs, inf_flags=None):
    return _verify("blsmi_g1pubs_verify_batch", 1, False, _msg_head(msgs), len(msgs), pks, sigs, inf_flags)


# ---- randomised batch verification (blsmi 0.8): one pairing check per batch, per-tuple verdicts only when it fails ---------------
def g2pubs_verify_batch_rlc(msgs, pks, sigs, inf_flags=None, scalars=None):
    """blsmi_g2pubs_verify_batch_rlc -> (ok, bitmap, combined): verify_batch's verdicts from one combined pairing check (combined == 1)
    or, when it fails, from the per-tuple path (combined == 0).  scalars: n nonzero 64-bit integers, or None (the library draws them)."""
    return _verify("blsmi_g2pubs_verify_batch_rlc", 0, False, _msg_head(msgs), len(msgs), pks, sigs, inf_flags, True, scalars)


def g1pubs_verify_batch_rlc(msgs, pks, sigs, inf_flags=None, scalars=None):
    return _verify("blsmi_g1pubs_verify_batch_rlc", 1, False, _msg_head(msgs), len(msgs), pks, sigs, inf_flags, True, scalars)


def g1pubs_verify_with_domain_batch_rlc(msgs32, domain8, pks, sigs, inf_flags=None, scalars=None):
    """-> (ok, combined)"""
    ok, _, comb = _verify("blsmi_g1pubs_verify_with_domain_batch_rlc", 1, False, _domain_head(msgs32, domain8), len(msgs32), pks, sigs, inf_flags, True, scalars, bitmap=False)
    return ok, comb


def verify_serialized_batch(group, msgs, pks, sigs, check_subgroup=True):
    """Deserialize + Verify in one device pass: compressed keys / signatures as Serialize() emits them.
    Returns (ok, err_pk, err_sig); err_* are the per-element deserialisation error codes (0 = fine)."""
    n = len(msgs)
    pkc, sgc = (96, 48) if group == "g2pubs" else (48, 96)
    ok = np.zeros(n, dtype=np.uint8); ep = np.zeros(n, dtype=np.uint8); es = np.zeros(n, dtype=np.uint8)
    _call("blsmi_%s_verify_serialized_batch" % _pubs(group), *_msg_head(msgs), _recs(pks, pkc * n, pad=True), _recs(sigs, sgc * n, pad=True), 1 if check_subgroup else 0,
          _p8(ok), _p8(ep), _p8(es), n)
    return ok.astype(bool), ep, es


def g1pubs_verify_with_domain_batch(msgs32, domain8, pks, sigs, inf_flags=None):
    return _verify("blsmi_g1pubs_verify_with_domain_batch", 1, False, _domain_head(msgs32, domain8), len(msgs32), pks, sigs, inf_flags, bitmap=False)[0]


def _verify_aggregate(name, kind, jac, head, n, pks, sig):
    """VerifyAggregate / VerifyAggregateCommon of one signature over n keys, through any of their host entry points; head: the leading
    arguments (_msg_head, _one_msg or the with-domain pair)"""
    pkb, sgb = _sizes(kind, jac)
    ok = C.c_int(0)
    _call(name, *head, _recs(pks, pkb * n, jac, pad=True), _recs(sig, sgb, jac), n, C.byref(ok))
    return bool(ok.value)


def g2pubs_verify_aggregate(msgs, pks, sig):
    return _verify_aggregate("blsmi_g2pubs_verify_aggregate", 0, False, _msg_head(msgs), len(msgs), pks, sig)


def g1pubs_verify_aggregate(msgs, pks, sig):
    return _verify_aggregate("blsmi_g1pubs_verify_aggregate", 1, False, _msg_head(msgs), len(msgs), pks, sig)


def g1pubs_verify_aggregate_with_domain(msgs32, domain8, pks, sig):
    return _verify_aggregate("blsmi_g1pubs_verify_aggregate_with_domain", 1, False, _domain_head(msgs32, domain8, 1), len(msgs32), pks, sig)


def g2pubs_verify_aggregate_common(msg, pks, sig, n):
    return _verify_aggregate("blsmi_g2pubs_verify_aggregate_common", 0, False, _one_msg(msg), n, pks, sig)


def g1pubs_verify_aggregate_common(msg, pks, sig, n):
    return _verify_aggregate("blsmi_g1pubs_verify_aggregate_common", 1, False, _one_msg(msg), n, pks, sig)


def g1pubs_verify_aggregate_common_with_domain(msg32, domain8, pks, sig, n):
    return _verify_aggregate("blsmi_g1pubs_verify_aggregate_common_with_domain", 1, False, (_p8(_u8(msg32, 32)), _p8(_u8(domain8, 8))), n, pks, sig)


def aggregate_partial(group, msgs, pks):
    """Shard-level half of VerifyAggregate: (prod_i MillerLoop(H(m_i), pk_i) as (72,) uint64 in the wire format,
    True if some key was the point at infinity)."""
    n = len(msgs)
    out = np.zeros(72, dtype=np.uint64)
    bad = C.c_int(0)
    _call("blsmi_%s_aggregate_partial" % _pubs(group), *_msg_head(msgs), _recs(pks, (192 if group == "g2pubs" else 96) * n, pad=True), n, _p64(out), C.byref(bad))
    return out, bool(bad.value)


def fq12_product(vals):
    x = np.ascontiguousarray(vals, dtype=np.uint64).reshape(-1, 72)
    out = np.zeros(72, dtype=np.uint64)
    _call("blsmi_fq12_product", _p64(x), x.shape[0], _p64(out))
    return out


# ---- wire format -----------------------------------------------------------------------------------
def _decompress(name, ib, ob, data, n, check):
    out = np.zeros((n, ob), dtype=np.uint8)
    inf = np.zeros(n, dtype=np.uint8)
    err = np.zeros(n, dtype=np.uint8)
    _call(name, _recs(data, ib * n), int(check), _p8(out.reshape(-1)), _p8(inf), _p8(err), n)
    return out, inf.astype(bool), err


def g1_decompress_batch(data, n, check_subgroup=True):
    return _decompress("blsmi_g1_decompress_batch", 48, 96, data, n, check_subgroup)


def g2_decompress_batch(data, n, check_subgroup=True):
    return _decompress("blsmi_g2_decompress_batch", 96, 192, data, n, check_subgroup)


def _compress(name, ib, ob, pts, n, in_inf):
    out = np.zeros((n, ob), dtype=np.uint8)
    _call(name, _recs(pts, ib * n), _flags(in_inf, n), _p8(out.reshape(-1)), n)
    return out


def g1_compress_batch(pts, n, in_inf=None):
    return _compress("blsmi_g1_compress_batch", 96, 48, pts, n, in_inf)


def g2_compress_batch(pts, n, in_inf=None):
    return _compress("blsmi_g2_compress_batch", 192, 96, pts, n, in_inf)


# ---- unit-level device ops (parity tests) -------------------------------------------------------------
OPS = dict(FQ_MUL=1, FQ_SQR=2, FQ_ADD=3, FQ_SUB=4, FQ_NEG=5, FQ_INV=6, FQ_SQRT=7, FQ_DBL=8, FQ_CMP=9, FQ_PARITY=10, FQ_LAZY=11,
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
    _call("blsmi_debug_g2_prepare", _p8(_u8(g2_aff, 192)) if g2_aff is not None else None, mode, _p64(out))
    return out.reshape(68, 3, 12)


def debug_hash_tail(kind, pts, n):
    """the level program behind a small-batch hash: mapped points -> (hash points (n, 96|192) uint8, good (n,) uint8)"""
    rec, hb = (384 if kind == 1 else 192), (96 if kind == 0 else 192)
    out = np.zeros((n, hb), dtype=np.uint8); good = np.zeros(n, dtype=np.uint8)
    _call("blsmi_debug_hash_tail", kind, _recs(pts, rec * n), _p8(out.reshape(-1)), _p8(good), n)
    return out, good


def debug_hash_redo(kind, msgs, good, out, domain8=None):
    """re-hash the messages whose good byte is 0 into `out` (n, 96|192) uint8; returns the updated array"""
    n = len(msgs)
    hb = 96 if kind == 0 else 192
    o = np.ascontiguousarray(out, dtype=np.uint8).reshape(n, hb).copy()
    g = _u8(good, n)
    if kind == 2:
        head = _p8(_u8(b"".join(bytes(m) for m in msgs), 32 * n)), _p64(_u8(domain8, 8))      # (the domain travels in the offsets' place)
    else:
        head = _msg_head(msgs)
    _call("blsmi_debug_hash_redo", kind, *head, _p8(g), _p8(o.reshape(-1)), n)
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
    _call("blsmi_debug_lat_unit", which, _ptr(a, i32p), nin, n, _ptr(out, i32p) if nout else None, _p8(ok))
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
        bp = _p64(b)
    _call("blsmi_debug_op", op | (LANE_PAIR if lane_pair else 0) | (LANE_QUAD if lane_quad else 0) | (LANE_ROW if lane_row else 0), _p64(a), bp, _p64(out), _p8(flag), n)
    return out, (flag.copy() if raw_flag else flag.astype(bool))


# ---- the reference's in-memory points at the boundary (blsmi 0.6, include/blsmi.h "in-memory points") ------------------------
# bls.G1Projective = 18 x u64, bls.G2Projective = 36 x u64 (x, y, z; each FQ 6 little-endian u64 Montgomery limbs): 144 / 288 bytes.
G1_JAC_BYTES, G2_JAC_BYTES = 144, 288


def _jac_to_affine(name, jb, wb, jac, n):
    out = np.zeros(max(1, wb * n), dtype=np.uint8)
    inf = np.zeros(max(1, n), dtype=np.uint8)
    _call(name, _recs(jac, jb * n, True), _p8(out), _p8(inf), n)
    return out[:wb * n].tobytes(), inf[:n].astype(bool)


def g1_jac_to_affine_batch(jac, n):
    """G1Projective.ToAffine().SerializeBytes() for n in-memory points -> (n*96 wire bytes, infinity flags)"""
    return _jac_to_affine("blsmi_g1_jac_to_affine_batch", 144, 96, jac, n)


def g2_jac_to_affine_batch(jac, n):
    return _jac_to_affine("blsmi_g2_jac_to_affine_batch", 288, 192, jac, n)


def pairing_batch_jac(g1_jac, g2_jac, n):
    """bls.Pairing on n (G1Projective, G2Projective) pairs as the Go heap holds them -> (n, 72) uint64"""
    out = np.zeros((n, 72), dtype=np.uint64)
    _call("blsmi_pairing_batch_jac", _recs(g1_jac, 144 * n, True), _recs(g2_jac, 288 * n, True), _p64(out), n)
    return out


def _sum_jac(name, jb, pts, n):
    out = np.zeros(jb // 8, dtype=np.uint64)
    oinf = C.c_int(0)
    _call(name, _recs(pts, jb * n, True), n, _p64(out), C.byref(oinf))
    return out.tobytes(), bool(oinf.value)


def g1_sum_jac(pts, n):
    """sum of n in-memory G1 points -> (the sum as an in-memory point with z = 1, is_infinity)"""
    return _sum_jac("blsmi_g1_sum_jac", 144, pts, n)


def g2_sum_jac(pts, n):
    return _sum_jac("blsmi_g2_sum_jac", 288, pts, n)


def g2pubs_verify_batch_jac(msgs, pks, sigs):
    return _verify("blsmi_g2pubs_verify_batch_jac", 0, True, _msg_head(msgs), len(msgs), pks, sigs)


def g1pubs_verify_batch_jac(msgs, pks, sigs):
    return _verify("blsmi_g1pubs_verify_batch_jac", 1, True, _msg_head(msgs), len(msgs), pks, sigs)


def g1pubs_verify_with_domain_batch_jac(msgs32, domain8, pks, sigs):
    return _verify("blsmi_g1pubs_verify_with_domain_batch_jac", 1, True, _domain_head(msgs32, domain8), len(msgs32), pks, sigs, bitmap=False)[0]


def g2pubs_verify_batch_rlc_jac(msgs, pks, sigs, scalars=None):
    """blsmi_g2pubs_verify_batch_rlc_jac over in-memory points -> (ok, bitmap, combined)"""
    return _verify("blsmi_g2pubs_verify_batch_rlc_jac", 0, True, _msg_head(msgs), len(msgs), pks, sigs, None, True, scalars)


def g1pubs_verify_batch_rlc_jac(msgs, pks, sigs, scalars=None):
    return _verify("blsmi_g1pubs_verify_batch_rlc_jac", 1, True, _msg_head(msgs), len(msgs), pks, sigs, None, True, scalars)


def g1pubs_verify_with_domain_batch_rlc_jac(msgs32, domain8, pks, sigs, scalars=None):
    """-> (ok, combined)"""
    ok, _, comb = _verify("blsmi_g1pubs_verify_with_domain_batch_rlc_jac", 1, True, _domain_head(msgs32, domain8), len(msgs32), pks, sigs, None, True, scalars, bitmap=False)
    return ok, comb


def g2pubs_verify_aggregate_jac(msgs, pks, sig):
    return _verify_aggregate("blsmi_g2pubs_verify_aggregate_jac", 0, True, _msg_head(msgs), len(msgs), pks, sig)


def g1pubs_verify_aggregate_jac(msgs, pks, sig):
    return _verify_aggregate("blsmi_g1pubs_verify_aggregate_jac", 1, True, _msg_head(msgs), len(msgs), pks, sig)


def g1pubs_verify_aggregate_with_domain_jac(msgs32, domain8, pks, sig):
    return _verify_aggregate("blsmi_g1pubs_verify_aggregate_with_domain_jac", 1, True, _domain_head(msgs32, domain8, 1), len(msgs32), pks, sig)


def g2pubs_verify_aggregate_common_jac(msg, pks, sig, n):
    return _verify_aggregate("blsmi_g2pubs_verify_aggregate_common_jac", 0, True, _one_msg(msg), n, pks, sig)


def g1pubs_verify_aggregate_common_jac(msg, pks, sig, n):
    return _verify_aggregate("blsmi_g1pubs_verify_aggregate_common_jac", 1, True, _one_msg(msg), n, pks, sig)


def g1pubs_verify_aggregate_common_with_domain_jac(msg32, domain8, pks, sig, n):
    return _verify_aggregate("blsmi_g1pubs_verify_aggregate_common_with_domain_jac", 1, True, (_p8(_u8(msg32, 32)), _p8(_u8(domain8, 8))), n, pks, sig)


class PreparedKeysJac(PreparedKeys):
    """PreparedKeys made from n in-memory G2 points (blsmi_g2_prepared_create_jac)"""

    def __init__(self, g2_jac, n):  # (does not call the affine constructor)
        self._create("blsmi_g2_prepared_create_jac", _recs(g2_jac, 288 * n, True), n)


def g2pubs_verify_batch_prepared_jac(msgs, prepared, key_idx, sigs):
    """g2pubs.Verify x n over prepared keys, the signatures as in-memory G1 points"""
    n = len(msgs)
    ok = np.zeros(n, dtype=np.uint8)
    _call("blsmi_g2pubs_verify_batch_prepared_jac", *_msg_head(msgs), *_prepared(prepared, key_idx), _recs(sigs, 144 * n, True), _p8(ok), None, n)
    return ok.astype(bool)


def g2pubs_verify_aggregate_prepared_jac(msgs, prepared, key_idx, sig):
    return _verify_aggregate_prepared("blsmi_g2pubs_verify_aggregate_prepared_jac", True, msgs, prepared, key_idx, sig)


def pairing_batch_jac_dev(d_g1_jac, d_g2_jac, d_out, n, stream=0):
    _call("blsmi_pairing_batch_jac_dev", d_g1_jac, d_g2_jac, d_out, n, stream)


def verify_batch_jac_dev(group, d_msgs, d_off, d_pks_jac, d_sigs_jac, d_ok, n, stream=0):
    """group: "g2pubs" / "g1pubs" / "g1pubs_with_domain" (d_off = the 8-byte domain on the device)"""
    name = {"g2pubs": "blsmi_g2pubs_verify_batch_jac_dev", "g1pubs": "blsmi_g1pubs_verify_batch_jac_dev", "g1pubs_with_domain": "blsmi_g1pubs_verify_with_domain_batch_jac_dev"}[group]
    _call(name, d_msgs, d_off, d_pks_jac, d_sigs_jac, d_ok, n, stream)


def g1_mul_generator_batch_jac(scalars, n):
    """PrivToPub for g1pubs: k_i * G1 as (n, 144) bytes of bls.G1Projective records (z = 1; (0, 1, 0) for k = 0 mod r)"""
    return _mul_hashed("blsmi_g1_mul_generator_batch_jac", True, 144, (), n, scalars)


def g2_mul_generator_batch_jac(scalars, n):
    return _mul_hashed("blsmi_g2_mul_generator_batch_jac", True, 288, (), n, scalars)


def g2pubs_sign_batch_jac(msgs, sks):
    return _mul_hashed("blsmi_g2pubs_sign_batch_jac", True, 144, _msg_head(msgs), len(msgs), sks)


def g1pubs_sign_batch_jac(msgs, sks):
    return _mul_hashed("blsmi_g1pubs_sign_batch_jac", True, 288, _msg_head(msgs), len(msgs), sks)


def g1pubs_sign_with_domain_batch_jac(msgs32, domain8, sks):
    return _mul_hashed("blsmi_g1pubs_sign_with_domain_batch_jac", True, 288, _domain_head(msgs32, domain8), len(msgs32), sks)


# ---- committees (blsmi 0.9): segmented sums and batches of VerifyAggregateCommon ------------------------------------------------
def seg_offsets(sizes):
    """Segment sizes -> the m + 1 offsets (uint64) of the segmented entry points: [0, s0, s0 + s1, ...]"""
    off = np.zeros(len(sizes) + 1, dtype=np.uint64)
    if len(sizes):
        np.cumsum(np.asarray(sizes, dtype=np.uint64), out=off[1:])
    return off


def _seg_args(idx, seg_off):
    """-> (the m + 1 offsets, the pointer to the optional indices: NULL without them)"""
    so = np.ascontiguousarray(seg_off, dtype=np.uint64)
    ix = None if idx is None else np.ascontiguousarray(idx, dtype=np.uint32)
    return so, (_p32(ix) if ix is not None and ix.size else None)


def _sum_segmented(name, pb, pts, npk, idx, seg_off, in_inf=None, jac=False, weighted=False, scalars=None):
    """m segmented sums -> (m affine records of pb bytes, out_inf).  jac: over in-memory points (no infinity flags); weighted: the *_u64 forms"""
    so, pidx = _seg_args(idx, seg_off)
    m = so.size - 1
    args = (_recs(pts, pb // 2 * 3 * npk, True), npk) if jac else (_recs(pts, pb * npk, pad=True), _flags(in_inf, npk), npk)
    if weighted:
        pr = _scalars(scalars, npk)
        args += (pr if npk else None,)
    out = np.zeros(max(1, pb * m), dtype=np.uint8)
    oinf = np.zeros(max(1, m), dtype=np.uint8)
    _call(name, *args, pidx, _p64(so), m, _p8(out), _p8(oinf))
    return out[:pb * m].tobytes(), oinf[:m].copy()


def g1_sum_segmented(pts, npk, idx, seg_off, in_inf=None):
    """m sums of affine G1 points: segment j = pts[idx[k]] for seg_off[j] <= k < seg_off[j + 1] (idx None: k itself).
    -> (m*96 affine bytes, out_inf: 1 infinity, 0 otherwise)"""
    return _sum_segmented("blsmi_g1_sum_segmented", 96, pts, npk, idx, seg_off, in_inf)


def g2_sum_segmented(pts, npk, idx, seg_off, in_inf=None):
    return _sum_segmented("blsmi_g2_sum_segmented", 192, pts, npk, idx, seg_off, in_inf)


def g1_sum_segmented_jac(pts_jac, npk, idx, seg_off):
    """the same over in-memory G1 points (144 bytes each) -> affine records and flags"""
    return _sum_segmented("blsmi_g1_sum_segmented_jac", 96, pts_jac, npk, idx, seg_off, jac=True)


def g2_sum_segmented_jac(pts_jac, npk, idx, seg_off):
    return _sum_segmented("blsmi_g2_sum_segmented_jac", 192, pts_jac, npk, idx, seg_off, jac=True)


def sum_segmented_dev(group, d_pts, d_in_inf, npk, d_idx, d_seg_off, m, d_out, d_out_inf, stream=0):
    """device-pointer form: out_inf bytes 0 / 1 / 2 (2: the segment holds an index >= npk, record zeroed)"""
    _call("blsmi_%s_sum_segmented_dev" % _g12(group), d_pts, d_in_inf, npk, d_idx, d_seg_off, m, d_out, d_out_inf, stream)


def _agg_common_batch(name, kind, jac, head, pks, npk, idx, seg_off, sigs, rlc=False, scalars=None):
    """m VerifyAggregateCommon()s over committees of one registry of npk keys -> (m verdict bytes, bitmap) or, for the randomised forms (rlc:
    scalars in, combined out), (ok, bitmap, combined).  head: the leading arguments, one message per item or (_grouped_head) a table and indices"""
    so, pidx = _seg_args(idx, seg_off)
    m = so.size - 1
    pkb, sgb = _sizes(kind, jac)
    ok = np.zeros(max(1, m), dtype=np.uint8)
    bm = np.zeros(max(1, (m + 7) // 8), dtype=np.uint8)
    comb = C.c_int(0)
    args = head + (_recs(pks, pkb * npk, jac, pad=True), npk, pidx, _p64(so), _recs(sigs, sgb * m, jac, pad=not rlc))
    if not rlc:
        _call(name, *args, _p8(ok), _p8(bm), m)
        return ok[:m].copy(), bm[:(m + 7) // 8].copy()
    _call(name, *args, _scalars(scalars, m), _p8(ok), _p8(bm), m, C.byref(comb))
    return ok[:m].astype(bool), bm[:(m + 7) // 8].copy(), comb.value


def _domain_items(msgs32, domain8, seg_off):
    """the with-domain committee forms' two leading arguments: one 32-byte message per item as raw bytes, the domain"""
    return _recs(msgs32, 32 * (len(seg_off) - 1), pad=True), _p8(_u8(domain8, 8))


def g2pubs_verify_aggregate_common_batch(msgs, pks, npk, idx, seg_off, sigs):
    """item j: VerifyAggregateCommon(sigs[j], {pks[idx[k]] : seg_off[j] <= k < seg_off[j + 1]}, msgs[j]) -> (m verdict bytes, bitmap)"""
    return _agg_common_batch("blsmi_g2pubs_verify_aggregate_common_batch", 0, False, _msg_head(msgs), pks, npk, idx, seg_off, sigs)


def g1pubs_verify_aggregate_common_batch(msgs, pks, npk, idx, seg_off, sigs):
    return _agg_common_batch("blsmi_g1pubs_verify_aggregate_common_batch", 1, False, _msg_head(msgs), pks, npk, idx, seg_off, sigs)


def g1pubs_verify_aggregate_common_with_domain_batch(msgs32, domain8, pks, npk, idx, seg_off, sigs):
    return _agg_common_batch("blsmi_g1pubs_verify_aggregate_common_with_domain_batch", 1, False, _domain_items(msgs32, domain8, seg_off), pks, npk, idx, seg_off, sigs)


def g2pubs_verify_aggregate_common_batch_jac(msgs, pks, npk, idx, seg_off, sigs):
    """the same over in-memory keys (288 bytes) and signatures (144 bytes)"""
    return _agg_common_batch("blsmi_g2pubs_verify_aggregate_common_batch_jac", 0, True, _msg_head(msgs), pks, npk, idx, seg_off, sigs)


def g1pubs_verify_aggregate_common_batch_jac(msgs, pks, npk, idx, seg_off, sigs):
    return _agg_common_batch("blsmi_g1pubs_verify_aggregate_common_batch_jac", 1, True, _msg_head(msgs), pks, npk, idx, seg_off, sigs)


def g1pubs_verify_aggregate_common_with_domain_batch_jac(msgs32, domain8, pks, npk, idx, seg_off, sigs):
    return _agg_common_batch("blsmi_g1pubs_verify_aggregate_common_with_domain_batch_jac", 1, True, _domain_items(msgs32, domain8, seg_off), pks, npk, idx, seg_off, sigs)


def verify_aggregate_common_batch_dev(group, d_msgs, d_off_or_domain, d_pks, npk, d_idx, d_seg_off, d_sigs, d_ok, m, stream=0, domain=False):
    """device-pointer forms: group "g2pubs" / "g1pubs" (domain=True: d_msgs holds m*32 bytes, d_off_or_domain the 8-byte domain); verdicts in d_ok"""
    name = "blsmi_g2pubs_verify_aggregate_common_batch_dev" if group == "g2pubs" else \
        ("blsmi_g1pubs_verify_aggregate_common_with_domain_batch_dev" if domain else "blsmi_g1pubs_verify_aggregate_common_batch_dev")
    _call(name, d_msgs, d_off_or_domain, d_pks, npk, d_idx, d_seg_off, d_sigs, d_ok, m, stream)


# ---- grouped randomised batch verification and the weighted segmented sums (blsmi 0.11) ----------------------------------------------
def g2pubs_verify_batch_rlc_grouped(msgs, msg_idx, pks, sigs, inf_flags=None, scalars=None):
    """blsmi_g2pubs_verify_batch_rlc_grouped -> (ok, bitmap, combined): tuple i is (msgs[msg_idx[i]], pk_i, sig_i); the tuples of one message
    share one pairing of the combined check.  Verdicts as g2pubs_verify_batch_rlc on the expanded messages."""
    n = len(msg_idx)
    return _verify("blsmi_g2pubs_verify_batch_rlc_grouped", 0, False, _grouped_head(msgs, msg_idx, n), n, pks, sigs, inf_flags, True, scalars)


def g1pubs_verify_batch_rlc_grouped(msgs, msg_idx, pks, sigs, inf_flags=None, scalars=None):
    n = len(msg_idx)
    return _verify("blsmi_g1pubs_verify_batch_rlc_grouped", 1, False, _grouped_head(msgs, msg_idx, n), n, pks, sigs, inf_flags, True, scalars)


def g1pubs_verify_with_domain_batch_rlc_grouped(msgs32, domain8, msg_idx, pks, sigs, inf_flags=None, scalars=None):
    n = len(msg_idx)
    return _verify("blsmi_g1pubs_verify_with_domain_batch_rlc_grouped", 1, False, _grouped_head(msgs32, msg_idx, n, domain8), n, pks, sigs, inf_flags, True, scalars)


def g2pubs_verify_batch_rlc_grouped_jac(msgs, msg_idx, pks, sigs, scalars=None):
    """the same over in-memory points (288 / 144 bytes each)"""
    n = len(msg_idx)
    return _verify("blsmi_g2pubs_verify_batch_rlc_grouped_jac", 0, True, _grouped_head(msgs, msg_idx, n), n, pks, sigs, None, True, scalars)


def g1pubs_verify_batch_rlc_grouped_jac(msgs, msg_idx, pks, sigs, scalars=None):
    n = len(msg_idx)
    return _verify("blsmi_g1pubs_verify_batch_rlc_grouped_jac", 1, True, _grouped_head(msgs, msg_idx, n), n, pks, sigs, None, True, scalars)


def g1pubs_verify_with_domain_batch_rlc_grouped_jac(msgs32, domain8, msg_idx, pks, sigs, scalars=None):
    n = len(msg_idx)
    return _verify("blsmi_g1pubs_verify_with_domain_batch_rlc_grouped_jac", 1, True, _grouped_head(msgs32, msg_idx, n, domain8), n, pks, sigs, None, True, scalars)


def g1_sum_segmented_u64(pts, npk, scalars, idx, seg_off, in_inf=None):
    """m weighted sums of affine G1 points: segment j = sum scalars[idx[k]] * pts[idx[k]] for seg_off[j] <= k < seg_off[j + 1]; scalars: npk
    64-bit integers (zero allowed).  -> (m*96 affine bytes, out_inf)"""
    return _sum_segmented("blsmi_g1_sum_segmented_u64", 96, pts, npk, idx, seg_off, in_inf, weighted=True, scalars=scalars)


def g2_sum_segmented_u64(pts, npk, scalars, idx, seg_off, in_inf=None):
    return _sum_segmented("blsmi_g2_sum_segmented_u64", 192, pts, npk, idx, seg_off, in_inf, weighted=True, scalars=scalars)


# ---- pairing products (blsmi 0.10): many MillerLoop(items) + FinalExponentiation checks in one call -----------------------------
def _pprod_offsets(seg_off, np_):
    so = np.ascontiguousarray(seg_off, dtype=np.uint64).reshape(-1)
    if so.size < 1:
        raise ValueError("seg_off needs m + 1 entries")
    if so.size > 1 and int(so[-1]) != np_:
        raise ValueError("seg_off ends at %d, the call has %d pairs" % (int(so[-1]), np_))
    return so, so.size - 1


def _pprod(name, jac, g1, g2, seg_off, inf_flags=None):
    pb, qb = (144, 288) if jac else (96, 192)
    a, b = _u8(g1), _u8(g2)
    if a.size % pb or b.size != 2 * a.size:
        raise ValueError("expected np*%d and np*%d bytes, got %d and %d" % (pb, qb, a.size, b.size))
    n = a.size // pb
    so, m = _pprod_offsets(seg_off, n)
    out, one = np.zeros((m, 72), dtype=np.uint64), np.zeros(max(1, m), dtype=np.uint8)
    pts = (_recs(a, a.size, True), _recs(b, b.size, True)) if jac else (_p8(a), _p8(b), _flags(inf_flags, n))
    _call(name, *pts, n, _p64(so), m, _p64(out), _p8(one))
    return out, one[:m].copy()


def pairing_product_batch(g1_aff, g2_aff, seg_off, inf_flags=None):
    """item j = FinalExponentiation(MillerLoop({(P_k, Q_k) : seg_off[j] <= k < seg_off[j + 1]})) over affine records (96 / 192 bytes a
    point; inf_flags[k] bit 0 / 1: P_k / Q_k is the point at infinity) -> (values (m, 72) uint64, is_one (m,) uint8)"""
    return _pprod("blsmi_pairing_product_batch", False, g1_aff, g2_aff, seg_off, inf_flags)


def pairing_product_batch_jac(g1_jac, g2_jac, seg_off):
    """the same over in-memory points (144 / 288 bytes each, z == 0: infinity)"""
    return _pprod("blsmi_pairing_product_batch_jac", True, g1_jac, g2_jac, seg_off)


def pairing_product_batch_dev(d_g1, d_g2, np_, d_seg_off, m, d_out_fq12, d_is_one, d_inf_flags=0, stream=0, jac=False):
    """device-pointer forms (ints): jac=False affine records and optional flags, jac=True in-memory points; d_out_fq12 (m*576 bytes) or
    d_is_one (m bytes) may be 0, not both"""
    if jac:
        if d_inf_flags:
            raise ValueError("the in-memory form takes no flags: z == 0 is infinity")
        _call("blsmi_pairing_product_batch_jac_dev", d_g1, d_g2, np_, d_seg_off, m, d_out_fq12, d_is_one, stream)
    else:
        _call("blsmi_pairing_product_batch_dev", d_g1, d_g2, d_inf_flags, np_, d_seg_off, m, d_out_fq12, d_is_one, stream)


# ---- randomised batch verification that finds the bad tuples by blocks (blsmi 0.12) ---------------------------------------------------
def g2pubs_verify_batch_rlc_locate(msgs, pks, sigs, inf_flags=None, scalars=None, block=0):
    """blsmi_g2pubs_verify_batch_rlc_locate -> (ok, bitmap, combined, rechecked): g2pubs_verify_batch_rlc's total check; when it fails, one
    pairing equation per block of `block` tuples (0: automatic; else even, >= 2) and verify_batch's verdicts for the tuples of the failing
    blocks only -- `rechecked` of them."""
    return _verify("blsmi_g2pubs_verify_batch_rlc_locate", 0, False, _msg_head(msgs), len(msgs), pks, sigs, inf_flags, True, scalars, block)


def g1pubs_verify_batch_rlc_locate(msgs, pks, sigs, inf_flags=None, scalars=None, block=0):
    return _verify("blsmi_g1pubs_verify_batch_rlc_locate", 1, False, _msg_head(msgs), len(msgs), pks, sigs, inf_flags, True, scalars, block)


def g1pubs_verify_with_domain_batch_rlc_locate(msgs32, domain8, pks, sigs, inf_flags=None, scalars=None, block=0):
    return _verify("blsmi_g1pubs_verify_with_domain_batch_rlc_locate", 1, False, _domain_head(msgs32, domain8, 32), len(msgs32), pks, sigs, inf_flags, True, scalars, block)


def g2pubs_verify_batch_rlc_locate_jac(msgs, pks, sigs, scalars=None, block=0):
    """the same over in-memory points (288 / 144 bytes each)"""
    return _verify("blsmi_g2pubs_verify_batch_rlc_locate_jac", 0, True, _msg_head(msgs), len(msgs), pks, sigs, None, True, scalars, block)


def g1pubs_verify_batch_rlc_locate_jac(msgs, pks, sigs, scalars=None, block=0):
    return _verify("blsmi_g1pubs_verify_batch_rlc_locate_jac", 1, True, _msg_head(msgs), len(msgs), pks, sigs, None, True, scalars, block)


def g1pubs_verify_with_domain_batch_rlc_locate_jac(msgs32, domain8, pks, sigs, scalars=None, block=0):
    return _verify("blsmi_g1pubs_verify_with_domain_batch_rlc_locate_jac", 1, True, _domain_head(msgs32, domain8, 32), len(msgs32), pks, sigs, None, True, scalars, block)


# ---- grouped randomised batch verification that finds the bad tuples by cells (blsmi 0.13) ---------------------------------------------
def g2pubs_verify_batch_rlc_grouped_locate(msgs, msg_idx, pks, sigs, inf_flags=None, scalars=None, block=0):
    """blsmi_g2pubs_verify_batch_rlc_grouped_locate -> (ok, bitmap, combined, rechecked): g2pubs_verify_batch_rlc_grouped's total check over
    cells of at most `block` tuples of one message (0: automatic; else any value >= 1); when it fails, one pairing equation per cell and
    verify_batch's verdicts for the tuples of the failing cells only -- `rechecked` of them."""
    n = len(msg_idx)
    return _verify("blsmi_g2pubs_verify_batch_rlc_grouped_locate", 0, False, _grouped_head(msgs, msg_idx, n), n, pks, sigs, inf_flags, True, scalars, block)


def g1pubs_verify_batch_rlc_grouped_locate(msgs, msg_idx, pks, sigs, inf_flags=None, scalars=None, block=0):
    n = len(msg_idx)
    return _verify("blsmi_g1pubs_verify_batch_rlc_grouped_locate", 1, False, _grouped_head(msgs, msg_idx, n), n, pks, sigs, inf_flags, True, scalars, block)


def g1pubs_verify_with_domain_batch_rlc_grouped_locate(msgs32, domain8, msg_idx, pks, sigs, inf_flags=None, scalars=None, block=0):
    n = len(msg_idx)
    return _verify("blsmi_g1pubs_verify_with_domain_batch_rlc_grouped_locate", 1, False, _grouped_head(msgs32, msg_idx, n, domain8), n, pks, sigs, inf_flags, True, scalars, block)


def g2pubs_verify_batch_rlc_grouped_locate_jac(msgs, msg_idx, pks, sigs, scalars=None, block=0):
    """the same over in-memory points (288 / 144 bytes each)"""
    n = len(msg_idx)
    return _verify("blsmi_g2pubs_verify_batch_rlc_grouped_locate_jac", 0, True, _grouped_head(msgs, msg_idx, n), n, pks, sigs, None, True, scalars, block)


def g1pubs_verify_batch_rlc_grouped_locate_jac(msgs, msg_idx, pks, sigs, scalars=None, block=0):
    n = len(msg_idx)
    return _verify("blsmi_g1pubs_verify_batch_rlc_grouped_locate_jac", 1, True, _grouped_head(msgs, msg_idx, n), n, pks, sigs, None, True, scalars, block)


def g1pubs_verify_with_domain_batch_rlc_grouped_locate_jac(msgs32, domain8, msg_idx, pks, sigs, scalars=None, block=0):
    n = len(msg_idx)
    return _verify("blsmi_g1pubs_verify_with_domain_batch_rlc_grouped_locate_jac", 1, True, _grouped_head(msgs32, msg_idx, n, domain8), n, pks, sigs, None, True, scalars, block)


# ---- point validation (blsmi 0.14): on-curve and subgroup status of points in either form ----------------------------------------------
POINT_OK, POINT_INFINITY, POINT_NOT_ON_CURVE, POINT_NOT_IN_SUBGROUP = 0, 1, 3, 4   # BLSMI_POINT_* (3, 4: the decompression error codes)


def _check_batch(name, pb, pts, n, in_inf, check, jac=False):
    status = np.zeros(max(1, n), dtype=np.uint8)
    pts = (_recs(pts, pb // 2 * 3 * n, True),) if jac else (_recs(pts, pb * n, pad=True), _flags(in_inf, n))
    _call(name, *pts, int(check), _p8(status), n)
    return status[:n].copy()


def g1_check_batch(pts, n, in_inf=None, check=1):
    """IsOnCurve / IsInCorrectSubgroupAssumingOnCurve of n affine G1 records (96 bytes each; in_inf: optional infinity flags) -> (n,) uint8:
    0 good, 1 infinity, 3 not on the curve, 4 outside the subgroup.  check: 0 the curve equation only, 1 the endomorphism test, 2 r * P."""
    return _check_batch("blsmi_g1_check_batch", 96, pts, n, in_inf, check)


def g2_check_batch(pts, n, in_inf=None, check=1):
    return _check_batch("blsmi_g2_check_batch", 192, pts, n, in_inf, check)


def g1_check_batch_jac(jac, n, check=1):
    """the same over in-memory G1 points (144 bytes each, z == 0: infinity): no conversion to affine, no inversion"""
    return _check_batch("blsmi_g1_check_batch_jac", 96, jac, n, None, check, jac=True)


def g2_check_batch_jac(jac, n, check=1):
    return _check_batch("blsmi_g2_check_batch_jac", 192, jac, n, None, check, jac=True)


def check_batch_dev(group, d_pts, d_in_inf, n, d_status, jac=False, check=1, stream=0):
    """device-pointer form (ints): d_pts affine records, or in-memory points with jac=True (then d_in_inf must be 0).  The n status bytes are
    in d_status when the call returns (it synchronises); the caller's point buffers are only read."""
    if jac and d_in_inf:
        raise ValueError("the in-memory form takes no flags: z == 0 is infinity")
    _call("blsmi_%s_check_batch_dev" % _g12(group), d_pts, d_in_inf, int(bool(jac)), int(check), d_status, n, stream)


# ---- the wire format <-> in-memory points (blsmi 0.15) -----------------------------------------------------------------------------------
def _decompress_jac(name, ib, jb, data, n, check):
    out = np.zeros(max(1, n) * jb, dtype=np.uint8)
    inf = np.zeros(max(1, n), dtype=np.uint8)
    err = np.zeros(max(1, n), dtype=np.uint8)
    _call(name, _recs(data, ib * n, pad=True), int(check), _p64(out), _p8(inf), _p8(err), n)
    return out[:n * jb].reshape(n, jb), inf[:n].astype(bool), err[:n].copy()


def g1_decompress_batch_jac(data, n, check_subgroup=True):
    """DecompressG1(b).ToProjective() of n 48-byte encodings -> ((n, 144) uint8 in-memory records, infinity flags, error codes); the flags and
    codes are g1_decompress_batch's, the record of an infinity or of an encoding with an error is the reference's zero point (0, 1, 0)"""
    return _decompress_jac("blsmi_g1_decompress_batch_jac", 48, 144, data, n, check_subgroup)


def g2_decompress_batch_jac(data, n, check_subgroup=True):
    return _decompress_jac("blsmi_g2_decompress_batch_jac", 96, 288, data, n, check_subgroup)


def _compress_jac(name, jb, ob, jac, n):
    out = np.zeros((max(1, n), ob), dtype=np.uint8)
    _call(name, _recs(jac, jb * n, True), _p8(out.reshape(-1)), n)
    return out[:n]


def g1_compress_batch_jac(jac, n):
    """CompressG1(p.ToAffine()) of n in-memory G1 points (144 bytes each, z == 0: infinity) -> (n, 48) uint8, one call and one launch"""
    return _compress_jac("blsmi_g1_compress_batch_jac", 144, 48, jac, n)


def g2_compress_batch_jac(jac, n):
    return _compress_jac("blsmi_g2_compress_batch_jac", 288, 96, jac, n)


def decompress_batch_jac_dev(group, d_in, n, d_out_jac, d_out_inf, d_err, check_subgroup=True, stream=0):
    """device-pointer form (ints; d_out_inf may be 0): the records, flags and codes are in the caller's buffers when the call returns"""
    _call("blsmi_%s_decompress_batch_jac_dev" % _g12(group), d_in, int(check_subgroup), d_out_jac, d_out_inf, d_err, n, stream)


def compress_batch_jac_dev(group, d_pts_jac, n, d_out, stream=0):
    _call("blsmi_%s_compress_batch_jac_dev" % _g12(group), d_pts_jac, d_out, n, stream)


# ---- committee aggregates, randomised (blsmi 0.16): many VerifyAggregateCommon under one pairing equation -----------------------------
def _agg_common_batch_rlc(name, kind, jac, msgs, msg_idx, pks, npk, idx, seg_off, sigs, scalars, domain8=None):
    """-> (ok, bitmap, combined); msgs: the table of d messages, msg_idx: one index into it per item, the registry and the committees as
    _agg_common_batch takes them"""
    return _agg_common_batch(name, kind, jac, _grouped_head(msgs, msg_idx, len(seg_off) - 1, domain8), pks, npk, idx, seg_off, sigs, True, scalars)


def g2pubs_verify_aggregate_common_batch_rlc(msgs, msg_idx, pks, npk, idx, seg_off, sigs, scalars=None):
    """blsmi_g2pubs_verify_aggregate_common_batch_rlc -> (ok, bitmap, combined): item j is VerifyAggregateCommon(sigs[j], {pks[idx[k]] :
    seg_off[j] <= k < seg_off[j + 1]}, msgs[msg_idx[j]]); one pairing equation for all m (combined == 1) or, when it fails, the verdicts of
    g2pubs_verify_aggregate_common_batch (combined == 0).  scalars: m nonzero 64-bit integers, or None (the library draws them)."""
    return _agg_common_batch_rlc("blsmi_g2pubs_verify_aggregate_common_batch_rlc", 0, False, msgs, msg_idx, pks, npk, idx, seg_off, sigs, scalars)


def g1pubs_verify_aggregate_common_batch_rlc(msgs, msg_idx, pks, npk, idx, seg_off, sigs, scalars=None):
    return _agg_common_batch_rlc("blsmi_g1pubs_verify_aggregate_common_batch_rlc", 1, False, msgs, msg_idx, pks, npk, idx, seg_off, sigs, scalars)


def g1pubs_verify_aggregate_common_with_domain_batch_rlc(msgs32, domain8, msg_idx, pks, npk, idx, seg_off, sigs, scalars=None):
    return _agg_common_batch_rlc("blsmi_g1pubs_verify_aggregate_common_with_domain_batch_rlc", 1, False, msgs32, msg_idx, pks, npk, idx, seg_off, sigs, scalars, domain8)


def g2pubs_verify_aggregate_common_batch_rlc_jac(msgs, msg_idx, pks, npk, idx, seg_off, sigs, scalars=None):
    """the same over in-memory keys (288 bytes) and signatures (144 bytes)"""
    return _agg_common_batch_rlc("blsmi_g2pubs_verify_aggregate_common_batch_rlc_jac", 0, True, msgs, msg_idx, pks, npk, idx, seg_off, sigs, scalars)


def g1pubs_verify_aggregate_common_batch_rlc_jac(msgs, msg_idx, pks, npk, idx, seg_off, sigs, scalars=None):
    return _agg_common_batch_rlc("blsmi_g1pubs_verify_aggregate_common_batch_rlc_jac", 1, True, msgs, msg_idx, pks, npk, idx, seg_off, sigs, scalars)


def g1pubs_verify_aggregate_common_with_domain_batch_rlc_jac(msgs32, domain8, msg_idx, pks, npk, idx, seg_off, sigs, scalars=None):
    return _agg_common_batch_rlc("blsmi_g1pubs_verify_aggregate_common_with_domain_batch_rlc_jac", 1, True, msgs32, msg_idx, pks, npk, idx, seg_off, sigs, scalars, domain8)


def verify_aggregate_common_batch_rlc_dev(group, d_msgs, d_off_or_domain, d, d_msg_idx, d_pks, npk, d_idx, d_seg_off, d_sigs, d_ok, m, scalars=None, stream=0, domain=False):
    """device-pointer forms (ints): group "g2pubs" / "g1pubs" (domain=True: d_msgs holds d*32 bytes, d_off_or_domain the 8-byte domain); the m
    verdict bytes are in d_ok when the call returns; scalars stay on the host.  -> combined"""
    name = "blsmi_g2pubs_verify_aggregate_common_batch_rlc_dev" if group == "g2pubs" else \
        ("blsmi_g1pubs_verify_aggregate_common_with_domain_batch_rlc_dev" if domain else "blsmi_g1pubs_verify_aggregate_common_batch_rlc_dev")
    comb = C.c_int(0)
    _call(name, d_msgs, d_off_or_domain, d, d_msg_idx, d_pks, npk, d_idx, d_seg_off, d_sigs, _scalars(scalars, m), d_ok, m, C.byref(comb), stream)
    return comb.value


def debug_g2_sum_segmented_u64_pair(pts, npk, scalars, idx, seg_off, in_inf=None):
    """g2_sum_segmented_u64 with pass 1 through the lane-pair ladder (k_g2_segsum_chunk_u64_pair), for the parity test"""
    return _sum_segmented("blsmi_debug_g2_sum_segmented_u64_pair", 192, pts, npk, idx, seg_off, in_inf, weighted=True, scalars=scalars)


# ---- pairing products, randomised (blsmi 0.17): one equation for a batch of pairing products over a table of G2 points -------------
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
        pix = None
    else:
        pix = _msg_idx(q_idx, n)
        if n == 0:                                                         # (a table without pairs: the pointer still says "indexed")
            pix = _p32(np.zeros(1, dtype=np.uint32))
    pr = _scalars(scalars, m)
    one = np.zeros(max(1, m), dtype=np.uint8)
    comb, nre = C.c_int(0), C.c_size_t(0)
    tail = (pr, _p8(one), C.byref(comb)) if block is None else (pr, block, _p8(one), C.byref(comb), C.byref(nre))
    pts = (_recs(a, a.size, True), _recs(t, t.size, True)) if jac else (_p8(a), _flags(inf_flags, n), _p8(t))
    _call(name, *pts, nq, pix, n, _p64(so), m, *tail)
    return (one[:m].copy(), comb.value) if block is None else (one[:m].copy(), comb.value, nre.value)


def _pprod_rlc_dev(name, points, nq, d_q_idx, np_, d_seg_off, m, d_is_one, scalars, stream, block=None):
    """the device-pointer forms; points: (d_g1, d_inf_flags, d_g2_tab) or, for in-memory points, (d_g1_jac, d_g2_tab_jac).  block None: the
    forms of 0.17 -> combined; the caller's `block`: those of 0.18 -> (combined, rechecked)"""
    pr = _scalars(scalars, m)
    comb, nre = C.c_int(0), C.c_size_t(0)
    out = (d_is_one, C.byref(comb)) if block is None else (_block(block), d_is_one, C.byref(comb), C.byref(nre))
    _call(name, *points, nq, d_q_idx, np_, d_seg_off, m, pr, *out, stream)
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
    _call("blsmi_fr_wsum_segmented_u64", _p8(v), ncol, _p64(w) if n else None, _p64(so), nseg, _p8(out.reshape(-1)))
    return out


def fr_wsum_segmented_u64_dev(d_vals, ncol, d_weights, d_seg_off, nseg, d_out, stream=0):
    """device-pointer form (ints); the nseg * (ncol + 1) scalars are in d_out when the call returns"""
    _call("blsmi_fr_wsum_segmented_u64_dev", d_vals, ncol, d_weights, d_seg_off, nseg, d_out, stream)


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
    pr = _scalars(scalars, m)
    block = _block(block)
    ok = np.zeros(max(1, m), dtype=np.uint8)
    comb, nre = C.c_int(0), C.c_size_t(0)
    k1, k2, a, b = (_recs(v, v.size, jac) for v in (k1, k2, a, b))
    _call(name, k1, k2, nin, a, b, _p8(x), m, pr, block, _p8(ok), C.byref(comb), C.byref(nre))
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
    pr = _scalars(scalars, m)
    comb, nre = C.c_int(0), C.c_size_t(0)
    _call(name, d_vk_g1, d_vk_g2, nin, d_proof_g1, d_proof_g2, d_inputs, m, pr, _block(block), d_ok, C.byref(comb), C.byref(nre), stream)
    return comb.value, nre.value


def groth16_verify_batch_dev(d_vk_g1, d_vk_g2, nin, d_proof_g1, d_proof_g2, d_inputs, m, d_ok, scalars=None, block=0, stream=0):
    """device-pointer form (ints) over affine records; the m verdict bytes are in d_ok when the call returns; scalars stay on the host.
    -> (combined, rechecked)"""
    return _groth16_dev("blsmi_groth16_verify_batch_dev", d_vk_g1, d_vk_g2, nin, d_proof_g1, d_proof_g2, d_inputs, m, d_ok, scalars, block, stream)


def groth16_verify_batch_jac_dev(d_vk_g1_jac, d_vk_g2_jac, nin, d_proof_g1_jac, d_proof_g2_jac, d_inputs, m, d_ok, scalars=None, block=0, stream=0):
    """device-pointer form over in-memory points -> (combined, rechecked)"""
    return _groth16_dev("blsmi_groth16_verify_batch_jac_dev", d_vk_g1_jac, d_vk_g2_jac, nin, d_proof_g1_jac, d_proof_g2_jac, d_inputs, m, d_ok, scalars, block, stream)
