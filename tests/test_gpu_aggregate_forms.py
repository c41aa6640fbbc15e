"""-m gpu: every VerifyAggregate form of the C ABI over ONE seeded workload per package, verdicts from the oracle alone.

Forms: host affine, *_jac, *_dev, *_with_domain, *_with_domain_dev, *_with_domain_jac, and for g2pubs *_prepared, *_prepared_dev,
*_prepared_jac with and without key_idx; aggregate_partial finished by the oracle's final exponentiation.  Sizes 0, 1, 2 and 65 (more
than one wave, an odd product tree).  Cases: valid; aggregate tampered; one wrong key; two equal messages; an empty message; a key at
infinity; the signature at infinity; valid and duplicate again under set_option("dup_force_sort", 1).  In the duplicate and empty cases
the aggregate is a correct signature of the messages as they stand, so the reference's duplicate rule (g2pubs/bls.go:245-261) alone
decides -- and the *WithDomain forms, which have no such rule (g1pubs/bls.go:300-311), must say True.  The expected verdict of every
case is oracle/refcpu's verify_aggregate (pyref.py's twin; a point at infinity, where the reference panics, gives 0), never another
form's.  The host form's device screen runs above 4 096 messages only: one case of 4 097."""
import hashlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from gpu_common import P, RC, g1_to_jac, g2_to_jac, pack, sk_bytes

pytestmark = pytest.mark.gpu
SIZES = (0, 1, 2, 65)
NK = 66                                                                    # 65 signers and one key that signs nothing
DOMAIN = bytes(range(1, 9))
CASES = ("valid", "tampered", "wrong_key", "dup", "empty", "key_inf", "sig_inf")


@pytest.fixture(scope="module")
def eng():
    from bls_amd import engine
    engine.init(0)
    return engine


def _dev(x):
    import torch
    a = np.frombuffer(x, dtype=np.uint8).copy() if isinstance(x, (bytes, bytearray)) else np.array(x)
    if a.dtype in (np.uint64, np.uint32):
        a = a.view(np.int64 if a.dtype == np.uint64 else np.int32)
    return torch.from_numpy(a).to(torch.device("cuda", 0))


class Pkg:
    """One package's keys, messages and per-message signatures, all from the oracle; kind: g2pubs, g1pubs or g1pubs_domain."""

    def __init__(self, kind, seed):
        self.kind = kind
        self.g2 = kind == "g2pubs"
        self.domain = kind == "g1pubs_domain"
        self.o = RC.g2pubs if self.g2 else RC.g1pubs
        self.pkb, self.sgb = (192, 96) if self.g2 else (96, 192)
        xs = P.XORShift(seed)
        self.sks = [sk_bytes(xs) for _ in range(NK)]
        self.pks = [self.o.priv_to_pub(sk) for sk in self.sks]
        raw = [b"aggregate form %d" % i + bytes(i % 5) for i in range(NK)]   # ragged lengths
        self.msgs = [hashlib.sha256(m).digest() for m in raw] if self.domain else raw
        self.sigs = [self.sign(m, i) for i, m in enumerate(self.msgs)]

    def sign(self, m, i):
        return RC.g1pubs.sign_with_domain(m, self.sks[i], DOMAIN) if self.domain else self.o.sign(m, self.sks[i])

    def sum(self, sigs):
        if not sigs:
            return bytes(self.sgb)
        s = (RC.g1_sum if self.g2 else RC.g2_sum)(b"".join(sigs), len(sigs))
        return s if s is not None else bytes(self.sgb)

    def case(self, name, n):
        """(msgs, pks, key indices into self.pks + [infinity], aggregate signature), or None where the case needs more tuples"""
        msgs, idx, sigs = list(self.msgs[:n]), list(range(n)), list(self.sigs[:n])
        if name == "tampered":
            sigs = sigs + [self.sigs[NK - 1]]
        elif name == "sig_inf":
            sigs = []
        elif n == 0 or (name == "dup" and n < 2) or (name == "empty" and self.domain):
            return None if name != "valid" else (msgs, [], idx, self.sum(sigs))
        elif name == "wrong_key":
            idx[n - 1] = NK - 1
        elif name == "dup":
            msgs[n - 1] = msgs[0]; sigs[n - 1] = self.sign(msgs[0], n - 1)
        elif name == "empty":
            msgs[n // 2] = b""; sigs[n // 2] = self.sign(b"", n // 2)
        elif name == "key_inf":
            idx[n // 2] = NK
        keys = self.pks + [bytes(self.pkb)]
        return msgs, [keys[i] for i in idx], idx, self.sum(sigs)

    def expect(self, msgs, pks, sig):
        """The oracle's VerifyAggregate.  It has no record for the point at infinity -- the reference panics in MillerLoop there
        (pairing.go:17-26), and the library's documented verdict for a panic is 0 (include/blsmi.h) -- so such a case is False by that rule."""
        if sig == bytes(self.sgb) or bytes(self.pkb) in pks:
            return False
        if self.domain:
            return RC.g1pubs.verify_aggregate_with_domain(sig, pks, msgs, DOMAIN)
        return self.o.verify_aggregate(sig, pks, msgs)


@pytest.fixture(scope="module")
def pkgs():
    return {k: Pkg(k, 9100 + i) for i, k in enumerate(("g2pubs", "g1pubs", "g1pubs_domain"))}


@pytest.fixture(scope="module")
def tables(eng, pkgs):
    """the g2pubs keys prepared once: tables 0 .. NK - 1, and table NK of the point at infinity"""
    g = pkgs["g2pubs"]
    t = eng.PreparedKeys(b"".join(g.pks) + bytes(192), NK + 1)
    yield t
    t.close()


def _jac_pk(pkg, pk):
    w = None if pk == bytes(pkg.pkb) else pk
    return g2_to_jac(w) if pkg.g2 else g1_to_jac(w)


def _jac_sig(pkg, sig):
    w = None if sig == bytes(pkg.sgb) else sig
    return g1_to_jac(w) if pkg.g2 else g2_to_jac(w)


def _forms(eng, pkg, tables, msgs, pks, idx, sig):
    """(name, verdict) of every form that takes this package's tuples"""
    n = len(msgs)
    pk_b, jpk_b, jsig = b"".join(pks), b"".join(_jac_pk(pkg, p) for p in pks), _jac_sig(pkg, sig)
    d_k = _dev(pk_b or b"\0")
    if pkg.domain:
        d_m, d_d = _dev(b"".join(msgs) or b"\0"), _dev(DOMAIN)
        yield "with_domain", eng.g1pubs_verify_aggregate_with_domain(msgs, DOMAIN, pk_b, sig)
        yield "with_domain_jac", eng.g1pubs_verify_aggregate_with_domain_jac(msgs, DOMAIN, jpk_b, jsig)
        yield "with_domain_dev", eng.verify_aggregate_with_domain_dev(d_m.data_ptr(), d_d.data_ptr(), d_k.data_ptr(), sig, n)
        return
    off = np.zeros(n + 1, dtype=np.uint64); off[1:] = np.cumsum([len(m) for m in msgs])
    d_m, d_o = _dev(b"".join(msgs) or b"\0"), _dev(off)
    host, jac = (eng.g2pubs_verify_aggregate, eng.g2pubs_verify_aggregate_jac) if pkg.g2 else (eng.g1pubs_verify_aggregate, eng.g1pubs_verify_aggregate_jac)
    yield "host", host(msgs, pk_b, sig)
    yield "jac", jac(msgs, jpk_b, jsig)
    yield "dev", eng.verify_aggregate_dev(pkg.kind, d_m.data_ptr(), d_o.data_ptr(), d_k.data_ptr(), sig, n)
    if not pkg.g2:
        return
    key_idx = np.array(idx, dtype=np.uint32)
    d_i = _dev(key_idx) if n else None
    yield "prepared[idx]", eng.g2pubs_verify_aggregate_prepared(msgs, tables, key_idx, sig)
    yield "prepared_jac[idx]", eng.g2pubs_verify_aggregate_prepared_jac(msgs, tables, key_idx, jsig)
    yield "prepared_dev[idx]", eng.g2pubs_verify_aggregate_prepared_dev(d_m.data_ptr(), d_o.data_ptr(), tables.ptr, d_i.data_ptr() if n else 0, sig, n)
    own = eng.PreparedKeys(pk_b, n) if n else tables                      # no key_idx: tuple t uses table t
    try:
        yield "prepared", eng.g2pubs_verify_aggregate_prepared(msgs, own, None, sig)
        yield "prepared_jac", eng.g2pubs_verify_aggregate_prepared_jac(msgs, own, None, jsig)
        yield "prepared_dev", eng.g2pubs_verify_aggregate_prepared_dev(d_m.data_ptr(), d_o.data_ptr(), own.ptr, 0, sig, n)
    finally:
        if n:
            own.close()


def _check_case(eng, pkg, tables, name, n):
    c = pkg.case(name, n)
    if c is None:
        return 0
    msgs, pks, idx, sig = c
    want = pkg.expect(msgs, pks, sig)
    got = dict(_forms(eng, pkg, tables, msgs, pks, idx, sig))
    print(pkg.kind, n, name, "oracle", want, got)
    assert got and all(v is want for v in got.values()), (pkg.kind, n, name, want, got)
    return len(got)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["g2pubs", "g1pubs", "g1pubs_domain"])
def test_every_form_gives_the_oracles_verdict(eng, pkgs, tables, kind, n):
    pkg = pkgs[kind]
    ran = sum(_check_case(eng, pkg, tables, name, n) for name in CASES)
    assert ran >= 2 * (3 if kind != "g2pubs" else 9)                       # at least the valid and the tampered case, through every form
    if n == 65:                                                            # the cases are what they claim to be: the rule alone rejects
        for name, rule in (("valid", True), ("dup", kind == "g1pubs_domain"), ("empty", False)):
            c = pkg.case(name, n)
            if c is not None:
                assert pkg.expect(c[0], c[1], c[3]) is rule


@pytest.mark.parametrize("n", [2, 65])
@pytest.mark.parametrize("kind", ["g2pubs", "g1pubs"])
def test_forms_under_dup_force_sort(eng, pkgs, tables, kind, n):
    """the duplicate screen's fallback, the reference's sort, on every call (the device-pointer forms fetch the messages for it)"""
    eng.set_option("dup_force_sort", 1)
    try:
        assert _check_case(eng, pkgs[kind], tables, "valid", n) and _check_case(eng, pkgs[kind], tables, "dup", n)
    finally:
        eng.set_option("dup_force_sort", 0)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["g2pubs", "g1pubs"])
def test_aggregate_partial_finished_by_the_oracle(eng, pkgs, kind, n):
    """FE(aggregate_partial) == prod_i e(H(m_i), pk_i), the right-hand side of the reference's VerifyAggregate, computed by the oracle"""
    pkg = pkgs[kind]
    msgs, pks = pkg.msgs[:n], pkg.pks[:n]
    part, bad = eng.aggregate_partial(kind, msgs, b"".join(pks))
    assert bad is False
    got = RC.final_exponentiation(part)[1]
    h = [(RC.hash_g1 if pkg.g2 else RC.hash_g2)(m) for m in msgs]
    g1s, g2s = (h, pks) if pkg.g2 else (pks, h)
    want = RC.final_exponentiation(RC.miller_loop(b"".join(g1s), b"".join(g2s), n))[1] if n else pack([1] + [0] * 11)   # no tuples: 1
    assert np.array_equal(np.asarray(got, dtype=np.uint64).reshape(-1), np.asarray(want, dtype=np.uint64).reshape(-1))
    if n:
        _, bad = eng.aggregate_partial(kind, msgs, b"".join(pks[:n - 1]) + bytes(pkg.pkb))
        assert bad is True                                                 # a key at infinity


@pytest.mark.parametrize("kind", ["g2pubs", "g1pubs"])
def test_host_form_device_screen_at_4097(eng, kind):
    """Above DUP_INLINE_MAX = 4 096 the host form screens for duplicates on the device.  Oracle-made signatures over 4 097 distinct
    messages verify; with message 4096 set equal to message 0 the reference's rule says False -- with the old aggregate, where the pairing
    equation fails as well, and with position 4096 signed again, where the rule alone rejects (test_gpu_dup_rule.py: the whole corpus)."""
    n, nk = 4097, 16
    o, host, g2 = (RC.g2pubs, eng.g2pubs_verify_aggregate, True) if kind == "g2pubs" else (RC.g1pubs, eng.g1pubs_verify_aggregate, False)
    xs = P.XORShift(4097)
    sks = [sk_bytes(xs) for _ in range(nk)]
    pks = [o.priv_to_pub(sk) for sk in sks]
    msgs = [b"screened on the device %d" % i for i in range(n)]
    with ThreadPoolExecutor(8) as ex:                                      # (the oracle's C calls release the interpreter lock)
        sigs = list(ex.map(lambda i: o.sign(msgs[i], sks[i % nk]), range(n)))
    agg = (RC.g1_sum if g2 else RC.g2_sum)(b"".join(sigs), n)
    keys = b"".join(pks[i % nk] for i in range(n))
    for i in (0, n - 1):
        assert o.verify(msgs[i], pks[i % nk], sigs[i]) is True
    assert len(set(msgs)) == n
    assert host(msgs, keys, agg) is True
    dup = list(msgs); dup[4096] = dup[0]
    assert sorted(dup)[0] == sorted(dup)[1] or len(set(dup)) < n           # the reference's rule: equal neighbours after sorting
    assert host(dup, keys, agg) is False
    sigs[4096] = o.sign(dup[4096], sks[4096 % nk])                         # a correct aggregate of the messages as they stand
    assert o.verify(dup[4096], pks[4096 % nk], sigs[4096]) is True
    assert host(dup, keys, (RC.g1_sum if g2 else RC.g2_sum)(b"".join(sigs), n)) is False
