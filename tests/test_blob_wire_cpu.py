"""CPU side of the Fiat-Shamir challenge and the wire-byte blob batches (blsmi 0.23: blsmi_kzg_blob_challenge_batch[_dev],
blsmi_kzg_verify_blob_batch_wire[_dev]): the model of tests/blob_wire_cases.py against pinned values and against its second, block-wise
restatement; bls_amd/csrc/sha256_fs.h run natively under the address and undefined-behaviour sanitizers against the model; the declarations,
the exports, the unit's registration; the argument checks that come before any device work; the wrappers' own checks; the corpus itself."""
import ctypes as C
import hashlib
import os
import random
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from bls_amd import _native, engine, kzg
from blob_wire_cases import (EDGES, INF48, K, M, QUOTIENT_CASES, SEED, SPOILS, STATUS_OF_EDGE, WireCase, challenge, challenge_by_blocks, compress_record, decode, digest, digest_by_blocks,
                             padded_blocks, quotient_blob)
from cabi_common import CTYPES, _header_params, bound_argtypes
from kzg_cases import INF, R
from oracle import pyref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -3
CHALLENGE = ["blsmi_kzg_blob_challenge_batch", "blsmi_kzg_blob_challenge_batch_dev", "blsmi_debug_kzg_blob_challenge_form_dev"]
WIRE = ["blsmi_kzg_verify_blob_batch_wire", "blsmi_kzg_verify_blob_batch_wire_dev", "blsmi_debug_kzg_verify_blob_batch_wire_dev_serial"]
HEADING = "==== Fiat-Shamir challenge and KZG blob batches from wire bytes (blsmi 0.23)"
TYPES = dict(CTYPES, unsigned=C.c_uint)


@pytest.fixture(scope="module")
def lib():
    _native.build()
    return _native.load()


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def test_the_model_against_pinned_values():
    assert challenge(bytes(32 << 12), 12, INF48) == 0x04b7b22af63d2b2f1ced8d550560e5d1e4b01e355903dee22781e87826856096
    assert challenge(bytes(32), 0, INF48) == 0x530ec343e38830f92fe5d046fcb3616ec39746e06f27a57ed53dfae0129e57d7
    assert digest(bytes(32), 0, INF48) // R == 1                                 # that digest is >= r: one subtraction
    assert [digest(quotient_blob(v), 2, INF48) // R for v, _ in QUOTIENT_CASES] == [q for _, q in QUOTIENT_CASES] == [0, 1, 2]
    g = P.g1_compress(P.G1_GEN).hex()
    assert g.startswith("97f1d3a7") and g.endswith("db22c6bb") and len(g) == 96  # the standard encoding of the generator
    assert hashlib.sha256(b"abc").hexdigest() == "%064x" % _digest_of_message(b"abc")   # the compression function against FIPS 180-4's example


def _digest_of_message(msg):
    """SHA-256 of any message through the model's compression function (the padding written out here)"""
    from blob_wire_cases import _H0, compress
    padded = msg + b"\x80" + bytes((55 - len(msg)) % 64) + (8 * len(msg)).to_bytes(8, "big")
    h = _H0
    for at in range(0, len(padded), 64):
        h = compress(h, padded[at:at + 64])
    return int.from_bytes(b"".join(x.to_bytes(4, "big") for x in h), "big")


@pytest.mark.parametrize("k", [0, 1, 2, 4, 12])
def test_the_two_restatements_agree(k):
    rng = random.Random(k)
    n = 1 << k
    for blob, c48 in ((bytes(32 * n), INF48), (rng.randbytes(32 * n), rng.randbytes(48)), (b"\xff" * (32 * n), b"\xff" * 48)):
        blocks = padded_blocks(blob, k, c48)
        assert len(blocks) == (2 if n == 1 else n // 2 + 2) and all(len(b) == 64 for b in blocks)
        assert b"".join(blocks)[:32 * n + 80] == b"FSBLOBVERIFY_V1_" + n.to_bytes(16, "big") + blob + c48
        assert digest_by_blocks(blob, k, c48) == digest(blob, k, c48) and challenge_by_blocks(blob, k, c48) == challenge(blob, k, c48) < R


# ---- sha256_fs.h, natively -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fs_driver(tmp_path_factory):
    gpp = shutil.which("g++") or shutil.which("c++")
    assert gpp, "no C++ compiler"
    exe = str(tmp_path_factory.mktemp("sha256_fs") / "sha256_fs")
    subprocess.check_call([gpp, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "native", "sha256_fs.cc")])
    return exe


def _native_lines(exe, text):
    out = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout[-400:], out.stderr[-2000:])
    return out.stdout.splitlines()


def test_sha256_fs_under_sanitizers(fs_driver):
    rng = random.Random(23)
    jobs = []
    for k in (0, 1, 2, 4, 12):
        n = 1 << k
        for off in (0, 1, 4, 15):                                                # 16-byte aligned, odd, word-aligned only
            jobs.append((k, off, rng.randbytes(32 * n), rng.randbytes(48)))
        jobs.append((k, 0, bytes(32 * n), INF48))
        jobs.append((k, 7, b"\xff" * (32 * n), b"\xff" * 48))
    jobs += [(2, off, quotient_blob(v), INF48) for v, _ in QUOTIENT_CASES for off in (0, 3)]
    lines = _native_lines(fs_driver, "".join("hash %d %d %s %s\n" % (k, off, blob.hex(), c48.hex()) for k, off, blob, c48 in jobs))
    assert len(lines) == 2 * len(jobs)
    for at, (k, off, blob, c48) in enumerate(jobs):
        d, z = int(lines[2 * at], 16), int(lines[2 * at + 1], 16)
        assert (d, z) == (digest(blob, k, c48), challenge(blob, k, c48)), (k, off)
        assert z == d - (d // R) * R and z < R
    assert {digest(b, k, c) // R for k, _, b, c in jobs} == {0, 1, 2}           # every branch of the reduction was taken


@pytest.mark.parametrize("k", [0, 1, 2, 3, 12, 16])
def test_the_layout_names_the_bytes_of_the_model(fs_driver, k):
    """every word of every block, as sha256_fs.h names its source, against the blocks the model builds by hand from a blob and a commitment
    whose bytes are all different in every aligned word"""
    n = 1 << k
    blob = b"".join((2 * i + 1).to_bytes(4, "big") for i in range(8 * n))
    c48 = b"".join((0x80000000 | i).to_bytes(4, "big") for i in range(12))
    lines = _native_lines(fs_driver, "layout %d\n" % k)
    blocks = padded_blocks(blob, k, c48)
    assert int(lines[-1]) == len(blocks) and len(lines) == 16 * len(blocks) + 1
    for i, b in enumerate(blocks):
        for w in range(16):
            src, v = lines[16 * i + w].split()
            src, v = int(src), int(v, 16)
            want = b[4 * w:4 * w + 4]
            got = v.to_bytes(4, "big") if src == 0 else (blob if src == 1 else c48)[v:v + 4]
            assert got == want and src in (0, 1, 2) and (src == 0 or v % 4 == 0), (k, i, w)
            assert src == 0 or v + 4 <= (32 * n if src == 1 else 48), (k, i, w)  # nothing beyond either buffer is named


# ---- registration --------------------------------------------------------------------------------------------------------------------------
def test_declared_exported_and_typed(lib, tmp_path):
    declared = _native.declared_symbols()
    header = open(_native.HEADER).read()
    assert "0.23 adds" in header and header.index("0.23 adds") > header.index("0.22 adds")
    assert header.count(HEADING) == 1 and header.index(HEADING) > header.index("==== coset interpolation in Fr and KZG cell batches (blsmi 0.22)")
    assert header.rindex("/* ====") == header.index("/* " + HEADING)               # the new section is the last one
    exported = set(re.findall(r" T (blsmi_\w+)", subprocess.run(["nm", "-D", _native.SO_PATH], capture_output=True, text=True, check=True).stdout))
    assert exported == set(declared)
    sigs = _native.signatures()
    for s in CHALLENGE + WIRE:
        assert s in declared and s in exported and hasattr(lib, s) and s in sigs, s
        assert bound_argtypes(s) == [TYPES[t] for t in _header_params(header, s)], s
    twin, mine = _header_params(header, "blsmi_kzg_verify_blob_batch"), _header_params(header, WIRE[0])
    assert mine[-7:] == twin[-7:] and len(mine) == len(twin) - 2                 # m, scalars, block, ok, status, combined, rechecked; no order, no z
    assert _header_params(header, WIRE[1]) == _header_params(header, WIRE[2])
    for w in ("blob_challenge_batch", "blob_challenge_batch_dev", "verify_blob_batch_wire", "verify_blob_batch_wire_dev"):
        assert callable(getattr(kzg, w)) and getattr(kzg, w).__module__ == "bls_amd.kzg" and not hasattr(engine, w), w
    block = re.sub(r"\s*\n \*\s*", " ", header[header.index(HEADING):])
    for phrase in ("FSBLOBVERIFY_V1_", "N as 16 big-endian bytes", "hashed AS THEY ARE", "nothing is decoded", "up to two subtractions", "N / 2 + 2 compression blocks",
                   "log2n <= 16", "k_kzg_fs_split", "k_kzg_fs_lane", "ONE k_g1_decompress launch", "AFFINE records", "errC | errPi << 3 | noncanon << 6",
                   "ok[j] = 1 EXACTLY when status[j] == 0", "A well-formed infinity", "is a VALID point", "48 bytes of 0xff", "is CLEARED before stage 4",
                   "*combined = 1 exactly when", "*rechecked counts", "BLSMI_E_ARG", "a zero caller scalar", "m beyond 2^31 - 2", "m beyond 2^32 - 1",
                   "beyond a size_t", "nothing is written", "*rechecked = 0 on every early return", "No `block` value is refused", "buffers stay untouched",
                   "one device", "request combiner", "\"rlc_min\" does NOT apply", "What it does not change", "no Go shim", "profiles/r23_blob_wire.log"):
        assert phrase in block, phrase
    blob_block = header[header.index("m KZG blob proofs under one key: blsmi_kzg_verify_batch for a caller"):header.index(HEADING)]
    assert "blsmi_kzg_verify_blob_batch_wire (0.23, below)" in blob_block        # the sentence about Fiat-Shamir points at the new call
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src = tmp_path / "t.c"
    src.write_text('#include "blsmi.h"\nint main(void) { return blsmi_kzg_blob_challenge_batch(0, 12u, 0, 0, 0) + blsmi_kzg_blob_challenge_batch_dev(0, 12u, 0, 0, 0, 0)'
                   ' + blsmi_debug_kzg_blob_challenge_form_dev(0, 12u, 0, 0, 0, 1, 0)'
                   ' + blsmi_kzg_verify_blob_batch_wire(0, 0, 0, 12u, 0, 0, 0, 0, 0, 0, 0, 0, 0)'
                   ' + blsmi_kzg_verify_blob_batch_wire_dev(0, 0, 0, 12u, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)'
                   ' + blsmi_debug_kzg_verify_blob_batch_wire_dev_serial(0, 0, 0, 12u, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0); }\n')
    subprocess.check_call([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(_native.HEADER), str(src)])


def test_the_kernels_are_a_unit_of_the_build():
    unit_name = "k_kzg_fs.hip"
    assert unit_name in _native._UNITS and unit_name in _native._COST and unit_name not in _native._LIMBS28_UNITS
    gen_path = os.path.join(ROOT, "tools", "gen_kernel_decls.py")
    assert '"%s"' % unit_name in open(gen_path).read()
    kernels_h = open(os.path.join(_native.CSRC, "kernels.h")).read()
    for k in ("k_kzg_fs_lane", "k_kzg_fs_split", "k_kzg_wire_status", "k_kzg_wire_verdicts"):
        assert "__global__ void %s(" % k in kernels_h, k
    assert os.path.exists(os.path.join(_native.CSRC, "sha256_fs.h"))
    # kernels.h is what the generator writes: run it on a copy of the tree's sources
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copytree(os.path.join(ROOT, "tools"), os.path.join(tmp, "tools"), ignore=shutil.ignore_patterns("__pycache__"))
        os.makedirs(os.path.join(tmp, "bls_amd"))
        shutil.copytree(_native.CSRC, os.path.join(tmp, "bls_amd", "csrc"), ignore=shutil.ignore_patterns("build", "*.z", "*.bin", "__pycache__"))
        subprocess.run([sys.executable, os.path.join(tmp, "tools", "gen_kernel_decls.py")], check=True, capture_output=True)
        assert open(os.path.join(tmp, "bls_amd", "csrc", "kernels.h")).read() == kernels_h


def test_argument_checks_come_before_any_device_work(lib):
    """this machine has no device: anything but BLSMI_E_ARG / BLSMI_OK here would be the sign of device work"""
    buf = (C.c_uint8 * 4096)()
    a, p8 = C.addressof(buf), C.cast(buf, C.POINTER(C.c_uint8))
    ch, ch_dev, ch_form = (engine._fn(n) for n in CHALLENGE)
    for f, x, tail in ((ch, p8, ()), (ch_dev, a, (None,)), (ch_form, a, (1, None)), (ch_form, a, (0, None))):
        assert f(None, 4, x, x, 2, *tail) == f(x, 4, None, x, 2, *tail) == f(x, 4, x, None, 2, *tail) == E_ARG
        assert f(x, 17, x, x, 2, *tail) == f(x, 1 << 31, x, x, 2, *tail) == E_ARG                          # log2n > 16
        assert f(x, 0, x, x, 1 << 32, *tail) == E_ARG                                                    # m beyond 2^32 - 1
        assert f(None, 99, None, None, 0, *tail) == 0 and f(x, 4, x, x, 0, *tail) == 0                     # m = 0
    assert ch_form(a, 4, a, a, 2, 2, None) == ch_form(a, 4, a, a, 2, -1, None) == E_ARG                    # a form that is neither
    for name in WIRE:
        fn = engine._fn(name)
        dev = name != WIRE[0]
        x = a if dev else p8

        def call(g=x, h=x, polys=x, log2n=4, c=x, p=x, m=2, scalars=None, block=0, ok=x, st=x, want_nre=True):
            sc = (C.c_uint64 * len(scalars))(*scalars) if scalars else None
            comb, nre = C.c_int(7), C.c_size_t(7)
            tail = (None,) if dev else ()
            rc = fn(g, h, polys, log2n, c, p, m, sc, block, ok, st, C.byref(comb), C.byref(nre) if want_nre else None, *tail)
            return rc, comb.value, nre.value if want_nre else 0
        for block in (0, 1, 1 << 40):
            for null in ("g", "h", "polys", "c", "p", "ok"):
                assert call(block=block, **{null: None}) == (E_ARG, 0, 0), (name, null + " NULL")
                assert call(block=block, st=None, **{null: None}) == (E_ARG, 0, 0), (name, null + " NULL")
            assert call(log2n=17, block=block) == (E_ARG, 0, 0) and call(log2n=0xffffffff, block=block) == (E_ARG, 0, 0), (name, "log2n > 16")
            assert call(scalars=[5, 0], block=block) == (E_ARG, 0, 0), (name, "a zero scalar")
            assert call(m=(1 << 31) - 1, block=block) == (E_ARG, 0, 0), (name, "m beyond 2^31 - 2")
            assert call(m=1 << 32, block=block) == (E_ARG, 0, 0), (name, "m beyond 2^32 - 1")
            assert call(m=0, block=block) == (0, 0, 0), (name, "m = 0")
            assert call(g=None, h=None, polys=None, log2n=99, c=None, p=None, ok=None, st=None, m=0, block=block) == (0, 0, 0), (name, "m = 0, nothing else")
            assert call(ok=None, block=block, want_nre=False)[:2] == (E_ARG, 0), (name, "rechecked may be NULL")
    assert all(b == 0 for b in buf)                                              # nothing was written


def _no_device_or(call, check):
    try:
        out = call()
    except engine.BlsmiError as e:
        assert "(-1)" in str(e), e
    else:
        assert check(out), out


def test_python_wrappers_validate_and_marshal():
    assert kzg.blob_challenge_batch(b"", 12, b"").shape == (0, 32)
    for bad in (lambda: kzg.blob_challenge_batch(bytes(32 * 16), 4, bytes(47)),          # whole commitments
                lambda: kzg.blob_challenge_batch(bytes(32 * 15), 4, bytes(48)),          # N values per commitment
                lambda: kzg.blob_challenge_batch(bytes(32 * 16), 17, bytes(48)), lambda: kzg.blob_challenge_batch(bytes(32 * 16), -1, bytes(48)),
                lambda: kzg.blob_challenge_batch_dev(0, 17, 0, 0, 0)):
        with pytest.raises(ValueError):
            bad()
    _no_device_or(lambda: kzg.blob_challenge_batch(bytes(32 * 16 * 2), 4, bytes(96)), lambda z: (z.shape, z.dtype) == ((2, 32), np.uint8))
    kzg.blob_challenge_batch_dev(0, 4, 0, 0, 0)
    with pytest.raises(engine.BlsmiError) as ei:
        kzg.blob_challenge_batch_dev(0, 4, 0, 0, 2)                              # null pointers with m > 0
    assert "(-3)" in str(ei.value)
    f = kzg.verify_blob_batch_wire
    g, h, blobs = bytes(96), bytes(192 * 2), bytes(32 * 16 * 2)
    for bad in (lambda: f(bytes(95), h, blobs, 4, bytes(96), bytes(96)),         # the key has one G1 record
                lambda: f(g, bytes(192 * 3), blobs, 4, bytes(96), bytes(96)),    # ... and two G2 records
                lambda: f(g, h, blobs, 4, bytes(96), bytes(144)),                # one proof per commitment
                lambda: f(g, h, blobs, 4, bytes(95), bytes(95)),                 # whole points
                lambda: f(g, h, blobs[32:], 4, bytes(96), bytes(96)),            # N values per blob
                lambda: f(g, h, blobs, 17, bytes(96), bytes(96)),
                lambda: f(g, h, blobs, 4, bytes(96), bytes(96), scalars=[1]),    # one scalar per blob
                lambda: f(g, h, blobs, 4, bytes(96), bytes(96), block=-1)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(engine.BlsmiError) as ei:
        f(g, h, blobs, 4, bytes(96), bytes(96), scalars=[3, 0])                  # a zero scalar: the library refuses
    assert "(-3)" in str(ei.value)
    ok, st, comb, nre = f(g, h, b"", 12, b"", b"")                               # m = 0
    assert ok.shape == (0,) and st.shape == (0,) and st.dtype == np.uint8 and (comb, nre) == (0, 0) and f(g, h, b"", 12, b"", b"", status=False)[1] is None
    for kw in ({}, {"scalars": [1, 2]}, {"block": 2}, {"status": False}):
        _no_device_or(lambda: f(g, h, blobs, 4, bytes(96), bytes(96), **kw), lambda out: (out[0].shape, out[0].dtype) == ((2,), np.uint8))
    fd = kzg.verify_blob_batch_wire_dev
    assert fd(0, 0, 0, 12, 0, 0, 0, 0) == (0, 0) and fd(0, 0, 0, 12, 0, 0, 0, 0, d_status=0, scalars=[], block=2, stream=0) == (0, 0)
    with pytest.raises(engine.BlsmiError) as ei:
        fd(0, 0, 0, 12, 0, 0, 2, 0)
    assert "(-3)" in str(ei.value)
    with pytest.raises(ValueError):
        fd(0, 0, 0, 17, 0, 0, 0, 0)


# ---- the corpus --------------------------------------------------------------------------------------------------------------------------
def test_the_wire_corpus_by_big_integers():
    valid = WireCase(M, K, SEED, edge=EDGES)
    assert valid.status == [STATUS_OF_EDGE.get(j, 0) for j in range(M)]          # each edge has the intended status
    assert valid.verdicts() == [int(st == 0) for st in valid.status]
    assert all(eq in (1, None) for eq in valid.equation()) and valid.equation()[EDGES_AT("noncanon", EDGES)] == 1   # the v + r item holds mod r
    zero, const, ff = EDGES_AT("zero", EDGES), EDGES_AT("const", EDGES), EDGES_AT("ff", EDGES)
    assert valid.c48[zero] == valid.p48[zero] == INF48 and valid.verdicts()[zero] == 1 and valid.blobs[zero] == bytes(32 << K)
    assert valid.p48[const] == INF48 and valid.c48[const] != INF48 and valid.verdicts()[const] == 1
    assert valid.blobs[ff] == bytes(32 << K) and valid.c48[ff] == valid.p48[ff] == b"\xff" * 48 and valid.verdicts()[ff] == 0
    assert valid.C[ff] == valid.pi[ff] == INF                                    # what an unmasked call would take for infinity
    assert valid.expect(8) == (valid.verdicts(), valid.status, 1, 0)             # status != 0 alone fails no block
    for kind, spoil in SPOILS.items():
        c = WireCase(M, K, SEED, edge=EDGES, spoil=spoil)
        assert c.status == valid.status, kind
        assert [j for j in range(M) if c.verdicts()[j] != valid.verdicts()[j]] == sorted(spoil), kind   # each spoil flips exactly its items
        for j, how in spoil.items():
            assert (c.blobs[j] != valid.blobs[j]) == (how == "f") and (c.c48[j] != valid.c48[j]) == (how == "C") and (c.p48[j] != valid.p48[j]) == (how == "pi"), kind
            assert (c.z[j] != valid.z[j]) == (how in ("f", "C")), kind           # z moves with the blob and with the commitment
        ok, st, comb, nre = c.expect(8)
        assert comb == 0 and nre == sum(min(8, M - 8 * b) for b in {j // 8 for j in spoil}), kind
    two = SPOILS["two"]
    assert len({j // 8 for j in two}) == 2 and len(two) == 2                     # two spoils in different blocks
    assert compress_record(INF) == INF48 and decode(INF48) == (0, INF) and decode(b"\xff" * 48)[0] == 2


def EDGES_AT(kind, edges):
    return next(j for j, e in edges.items() if e == kind or (isinstance(e, tuple) and e[0] == kind))
