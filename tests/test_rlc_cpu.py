"""CPU side of the randomised batch verification (blsmi 0.8): the oracle composition the GPU tests (tests/test_gpu_rlc.py) expect, the six
prototypes in the header, and the shims' bindings."""
import hashlib
import os
import random
import re

import numpy as np

from oracle import pyref as P
from oracle import refcpu as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOS = ["blsmi_g2pubs_verify_batch_rlc", "blsmi_g1pubs_verify_batch_rlc", "blsmi_g1pubs_verify_with_domain_batch_rlc",
          "blsmi_g2pubs_verify_batch_rlc_jac", "blsmi_g1pubs_verify_batch_rlc_jac", "blsmi_g1pubs_verify_with_domain_batch_rlc_jac"]


def _fe(f):
    return RC.final_exponentiation(f)[1]


def _sk(i):
    return hashlib.sha256(b"cpu-rlc-%d" % i).digest()[:31].rjust(32, b"\0")


def _combined(msgs, pks, sigs, r):
    """g2pubs: e(sum r_i sig_i, G2gen) == prod e(r_i H(m_i), pk_i), from the oracle's primitives"""
    n = len(msgs)
    k = [int(x).to_bytes(32, "big") for x in r]
    S = RC.g1_sum(b"".join(RC.g1_mul(sigs[i], k[i]) for i in range(n)), n)
    lhs = _fe(RC.miller_loop(S, RC.g2_generator(), 1))
    rH = b"".join(RC.g1_mul(RC.hash_g1(msgs[i]), k[i]) for i in range(n))
    return np.array_equal(lhs, _fe(RC.miller_loop(rH, b"".join(pks), n)))


def _neg_g1(p):
    return p[:48] + ((P.Q - int.from_bytes(p[48:], "big")) % P.Q).to_bytes(48, "big")


def test_oracle_composition():
    n = 4
    msgs = [b"cpu rlc %d" % i for i in range(n)]
    pks = [RC.g2pubs.priv_to_pub(_sk(i)) for i in range(n)]
    sigs = [RC.g2pubs.sign(msgs[i], _sk(i)) for i in range(n)]
    rnd = random.Random(1)
    r = [rnd.randrange(1, 1 << 64) for _ in range(n)]
    assert _combined(msgs, pks, sigs, r)                                        # the honest batch holds
    D = RC.g1_mul(RC.g1_generator(), _sk(99))
    bad = list(sigs)
    bad[0] = RC.g1_sum(sigs[0] + D, 2)
    bad[1] = RC.g1_sum(sigs[1] + _neg_g1(D), 2)
    assert not RC.g2pubs.verify(msgs[0], pks[0], bad[0]) and not RC.g2pubs.verify(msgs[1], pks[1], bad[1])
    assert _combined(msgs, pks, bad, [1] * n)                                   # the cancelling pair holds under r = 1 ...
    assert not _combined(msgs, pks, bad, r)                                     # ... and not under random weights


def test_header_declares_the_prototypes():
    txt = open(os.path.join(ROOT, "include", "blsmi.h")).read()
    for fn in PROTOS:
        m = re.search(r"\bint %s\(([^;]*)\);" % fn, txt, flags=re.S)
        assert m, fn
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert "const uint64_t *scalars" in args and args.rstrip().endswith("int *combined"), fn
    assert re.search(r"#define BLSMI_E_RNG \(-6\)", txt)
    assert "BLSMI_OP_G1_MUL_U64 = 70" in txt


def test_shims_bind_the_jac_forms():
    g2 = open(os.path.join(ROOT, "shim", "g2pubs", "accel_cgo.go")).read()
    g1 = open(os.path.join(ROOT, "shim", "g1pubs", "accel_cgo.go")).read()
    assert "func VerifyBatchRandomized(msgs [][]byte, pubs []*PublicKey, sigs []*Signature) []bool" in g2
    assert "C.blsmi_g2pubs_verify_batch_rlc_jac(" in g2
    assert "func VerifyBatchRandomized(msgs [][]byte, pubs []*PublicKey, sigs []*Signature) []bool" in g1
    assert "func VerifyWithDomainBatchRandomized(msgs [][32]byte, pubs []*PublicKey, sigs []*Signature, domain [8]byte) []bool" in g1
    assert "C.blsmi_g1pubs_verify_batch_rlc_jac(" in g1 and "C.blsmi_g1pubs_verify_with_domain_batch_rlc_jac(" in g1
