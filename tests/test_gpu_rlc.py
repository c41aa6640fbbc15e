"""-m gpu: randomised batch verification (blsmi 0.8, blsmi_g?pubs_*verify*_batch_rlc[_jac]).  One combined pairing check per batch with
64-bit weights; verify_batch's per-tuple verdicts when it fails.  The expected combined verdict is composed from the oracle: hash, 64-bit
multiples (g1_mul / g2_mul with the scalar as 32 bytes), the signature sum, one Miller loop over the pair list, the final exponentiation."""
import ctypes
import hashlib
import os
import random
import re
import subprocess
import sys
import threading

import numpy as np
import pytest

from gpu_common import P, RC, g1_to_jac, g2_to_jac

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("g2pubs", "g1pubs", "domain")
DOMAIN = bytes(range(1, 9))
EDGE = [1, 1 << 63, (1 << 64) - 1, 2]


def _fe(f):
    return RC.final_exponentiation(f)[1]


def _default_rlc_min():
    return int(re.search(r'"rlc_min" \(BLSMI_RLC_MIN, default (\d+)\)', open(os.path.join(ROOT, "include", "blsmi.h")).read()).group(1))


@pytest.fixture(scope="module")
def eng():
    from bls_amd import engine
    engine.init(0)
    engine.set_option("rlc_min", 0)
    yield engine
    engine.set_option("rlc_min", _default_rlc_min())


def _sks(n, seed):
    return b"".join(hashlib.sha256(b"rlc-sk-%d-%d" % (seed, i)).digest()[:31].rjust(32, b"\0") for i in range(n))


def _msgs(kind, n, seed):
    if kind == "domain":
        return [hashlib.sha256(b"rlc-m-%d-%d" % (seed, i)).digest() for i in range(n)]
    return [b"rlc message %d/%d" % (seed, i) + b"x" * (i % 7) for i in range(n)]


def _batch(eng, kind, n, seed=0):
    """(msgs, pks (n, pkb), sigs (n, sgb)) of n valid tuples, signed on the device"""
    sks = _sks(n, seed)
    msgs = _msgs(kind, n, seed)
    if kind == "g2pubs":
        pks, _ = eng.g2_mul_generator_batch(sks, n)
        sigs, _ = eng.g2pubs_sign_batch(msgs, sks)
    elif kind == "g1pubs":
        pks, _ = eng.g1_mul_generator_batch(sks, n)
        sigs, _ = eng.g1pubs_sign_batch(msgs, sks)
    else:
        pks, _ = eng.g1_mul_generator_batch(sks, n)
        sigs, _ = eng.g1pubs_sign_with_domain_batch(msgs, DOMAIN, sks)
    pkb, sgb = (192, 96) if kind == "g2pubs" else (96, 192)
    return msgs, np.asarray(pks, np.uint8).reshape(n, pkb).copy(), np.asarray(sigs, np.uint8).reshape(n, sgb).copy()


def rlc(eng, kind, msgs, pks, sigs, inf=None, scalars=None):
    """-> (ok list, bitmap, combined)"""
    p, s = np.asarray(pks).tobytes(), np.asarray(sigs).tobytes()
    if kind == "domain":
        ok, comb = eng.g1pubs_verify_with_domain_batch_rlc(msgs, DOMAIN, p, s, inf, scalars)
        bm = np.packbits(np.asarray(ok, np.uint8), bitorder="little") if len(ok) else np.zeros(0, np.uint8)
        return [bool(x) for x in ok], bm, comb
    fn = eng.g2pubs_verify_batch_rlc if kind == "g2pubs" else eng.g1pubs_verify_batch_rlc
    ok, bm, comb = fn(msgs, p, s, inf, scalars)
    assert np.array_equal(bm, np.packbits(np.asarray(ok, np.uint8), bitorder="little")[:len(bm)])
    return [bool(x) for x in ok], bm, comb


def vb(eng, kind, msgs, pks, sigs, inf=None):
    p, s = np.asarray(pks).tobytes(), np.asarray(sigs).tobytes()
    if kind == "domain":
        return [bool(x) for x in eng.g1pubs_verify_with_domain_batch(msgs, DOMAIN, p, s, inf)]
    fn = eng.g2pubs_verify_batch if kind == "g2pubs" else eng.g1pubs_verify_batch
    return [bool(x) for x in fn(msgs, p, s, inf)[0]]


def oracle_verify(kind, m, pk, sig):
    pk, sig = bytes(pk), bytes(sig)
    if kind == "g2pubs":
        return RC.g2pubs.verify(m, pk, sig)
    if kind == "g1pubs":
        return RC.g1pubs.verify(m, pk, sig)
    return RC.g1pubs.verify_with_domain(m, pk, sig, DOMAIN)


def oracle_combined(kind, msgs, pks, sigs, r):
    """the combined equation with scalars r, composed from the oracle's primitives"""
    n = len(msgs)
    k32 = [int(x).to_bytes(32, "big") for x in r]
    if kind == "g2pubs":
        S = RC.g1_sum(b"".join(RC.g1_mul(bytes(sigs[i]), k32[i]) for i in range(n)), n)
        lhs = _fe(RC.miller_loop(S, RC.g2_generator(), 1))
        rH = b"".join(RC.g1_mul(RC.hash_g1(msgs[i]), k32[i]) for i in range(n))
        rhs = _fe(RC.miller_loop(rH, b"".join(bytes(p) for p in pks), n))
    else:
        S = RC.g2_sum(b"".join(RC.g2_mul(bytes(sigs[i]), k32[i]) for i in range(n)), n)
        lhs = _fe(RC.miller_loop(RC.g1_generator(), S, 1))
        rP = b"".join(RC.g1_mul(bytes(pks[i]), k32[i]) for i in range(n))
        H = b"".join(RC.hash_g2(msgs[i]) if kind == "g1pubs" else RC.hash_g2_with_domain(msgs[i], DOMAIN) for i in range(n))
        rhs = _fe(RC.miller_loop(rP, H, n))
    return np.array_equal(lhs, rhs)


def _neg(kind, pt):
    """-P of a wire record in the signature group"""
    b = bytearray(pt)
    offs = (48,) if kind == "g2pubs" else (96, 144)
    for o in offs:
        y = int.from_bytes(b[o:o + 48], "big")
        b[o:o + 48] = ((P.Q - y) % P.Q).to_bytes(48, "big")
    return bytes(b)


def _sig_add(kind, a, b):
    return (RC.g1_sum if kind == "g2pubs" else RC.g2_sum)(bytes(a) + bytes(b), 2)


def _sig_mul(kind, a, k):
    return (RC.g1_mul if kind == "g2pubs" else RC.g2_mul)(bytes(a), int(k).to_bytes(32, "big"))


def _rand_sig_point(kind, seed):
    k = hashlib.sha256(b"D%d" % seed).digest()[:31].rjust(32, b"\0")
    return RC.g1_mul(RC.g1_generator(), k) if kind == "g2pubs" else RC.g2_mul(RC.g2_generator(), k)


def _jac_forms(kind, pks, sigs, seed):
    rnd = random.Random(seed)
    if kind == "g2pubs":
        pj = b"".join(g2_to_jac(bytes(p), (rnd.randrange(1, P.Q), rnd.randrange(P.Q))) for p in pks)
        sj = b"".join(g1_to_jac(bytes(s), rnd.randrange(1, P.Q)) for s in sigs)
    else:
        pj = b"".join(g1_to_jac(bytes(p), rnd.randrange(1, P.Q)) for p in pks)
        sj = b"".join(g2_to_jac(bytes(s), (rnd.randrange(1, P.Q), rnd.randrange(P.Q))) for s in sigs)
    return pj, sj


def rlc_jac(eng, kind, msgs, pj, sj, scalars=None):
    if kind == "domain":
        ok, comb = eng.g1pubs_verify_with_domain_batch_rlc_jac(msgs, DOMAIN, pj, sj, scalars)
        return [bool(x) for x in ok], comb
    fn = eng.g2pubs_verify_batch_rlc_jac if kind == "g2pubs" else eng.g1pubs_verify_batch_rlc_jac
    ok, _, comb = fn(msgs, pj, sj, scalars)
    return [bool(x) for x in ok], comb


# ---- 1. all valid -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_all_valid_affine_and_in_memory(eng, kind):
    for n in (1, 3, 64, 1000, 4096):
        msgs, pks, sigs = _batch(eng, kind, n, seed=n)
        ok, _, comb = rlc(eng, kind, msgs, pks, sigs)
        assert comb == 1 and all(ok), (kind, n)
        assert ok == vb(eng, kind, msgs, pks, sigs), (kind, n)
        if n <= 1000:
            pj, sj = _jac_forms(kind, pks, sigs, n)
            okj, combj = rlc_jac(eng, kind, msgs, pj, sj)
            assert combj == 1 and all(okj), (kind, n, "in-memory")


# ---- 2. corruptions ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_corruptions_fall_back_to_per_tuple_verdicts(eng, kind):
    n = 64
    msgs, pks, sigs = _batch(eng, kind, n, seed=7)
    cases = []
    m = list(msgs); m[5] = hashlib.sha256(b"other").digest() if kind == "domain" else b"another message"
    cases.append((m, pks, sigs, {5}))                                           # wrong message
    p = pks.copy(); p[9] = pks[10]
    cases.append((msgs, p, sigs, {9}))                                          # wrong key
    s = sigs.copy(); s[20] = np.frombuffer(_rand_sig_point(kind, 1), np.uint8)
    cases.append((msgs, pks, s, {20}))                                          # tampered signature
    s = sigs.copy(); s[[30, 31]] = sigs[[31, 30]]
    cases.append((msgs, pks, s, {30, 31}))                                      # swapped signatures
    s = sigs.copy(); s[0] = sigs[1]; s[63] = np.frombuffer(_rand_sig_point(kind, 2), np.uint8); m2 = list(msgs); m2[40] = m[5]
    cases.append((m2, pks, s, {0, 40, 63}))                                     # several at once
    for (mm, pp, ss, bad) in cases:
        ok, bm, comb = rlc(eng, kind, mm, pp, ss)
        assert comb == 0, (kind, bad)
        assert ok == vb(eng, kind, mm, pp, ss), (kind, bad)
        for i in bad:
            assert ok[i] is False and oracle_verify(kind, mm[i], pp[i], ss[i]) is False, (kind, i)
        assert sum(ok) == n - len(bad)


# ---- 3. a cancelling pair: the plain sum is the honest aggregate, the weighted one is not ----------------------------------------
@pytest.mark.parametrize("kind", ("g2pubs", "g1pubs"))
def test_cancelling_pair_is_caught(eng, kind):
    n = 16
    msgs, pks, sigs = _batch(eng, kind, n, seed=11)
    D = _rand_sig_point(kind, 3)
    s = sigs.copy()
    s[2] = np.frombuffer(_sig_add(kind, sigs[2], D), np.uint8)
    s[7] = np.frombuffer(_sig_add(kind, sigs[7], _neg(kind, D)), np.uint8)
    ok, _, comb = rlc(eng, kind, msgs, pks, s)
    assert comb == 0 and not ok[2] and not ok[7] and sum(ok) == n - 2
    ok1, _, comb1 = rlc(eng, kind, msgs, pks, s, scalars=[1] * n)               # weights of 1: the attack goes through (why the weights exist)
    assert comb1 == 1 and all(ok1)


# ---- 4. the scalars are applied exactly --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_caller_scalars_applied_exactly(eng, kind):
    n = 8
    msgs, pks, sigs = _batch(eng, kind, n, seed=13)
    rnd = random.Random(5)
    r = EDGE + [rnd.randrange(1, 1 << 64) for _ in range(n - len(EDGE))]
    a, b = 2, 1                                                                  # r_a = 2^64 - 1, r_b = 2^63
    D = _rand_sig_point(kind, 4)
    s = sigs.copy()
    s[a] = np.frombuffer(_sig_add(kind, sigs[a], _sig_mul(kind, D, r[b])), np.uint8)
    s[b] = np.frombuffer(_sig_add(kind, sigs[b], _neg(kind, _sig_mul(kind, D, r[a]))), np.uint8)
    assert oracle_combined(kind, msgs, pks, s, r)
    assert not oracle_combined(kind, msgs, pks, s, [x ^ 4 for x in r])
    ok, _, comb = rlc(eng, kind, msgs, pks, s, scalars=r)
    assert comb == 1 and all(ok)
    ok, _, comb = rlc(eng, kind, msgs, pks, s)
    assert comb == 0 and not ok[a] and not ok[b] and sum(ok) == n - 2
    r2 = list(r); r2[0] = 3                                                      # a different weight elsewhere changes nothing ...
    assert rlc(eng, kind, msgs, pks, s, scalars=r2)[2] == 1
    r3 = list(r); r3[a] = r[a] - 1                                               # ... one bit less of r_a breaks it
    assert rlc(eng, kind, msgs, pks, s, scalars=r3)[2] == 0


def test_caller_scalars_bucket_msm(eng):
    """8 192 signatures: the signature sum runs the 64-bit bucket MSM, which must weight exactly as the ladders do"""
    kind, n = "g2pubs", 8192
    msgs, pks, sigs = _batch(eng, kind, n, seed=17)
    rnd = random.Random(9)
    r = [rnd.randrange(1, 1 << 64) for _ in range(n)]
    r[:4] = EDGE
    a, b = 2, 1
    D = _rand_sig_point(kind, 5)
    s = sigs.copy()
    s[a] = np.frombuffer(_sig_add(kind, sigs[a], _sig_mul(kind, D, r[b])), np.uint8)
    s[b] = np.frombuffer(_sig_add(kind, sigs[b], _neg(kind, _sig_mul(kind, D, r[a]))), np.uint8)
    ok, _, comb = rlc(eng, kind, msgs, pks, s, scalars=r)
    assert comb == 1 and all(ok)
    r[a] ^= 1 << 40
    ok, _, comb = rlc(eng, kind, msgs, pks, s, scalars=r)
    assert comb == 0 and not ok[a] and not ok[b] and sum(ok) == n - 2


# ---- 5. the 64-bit ladder against the oracle ------------------------------------------------------------------------------------------
def _off_subgroup_g1(seed):
    """an affine point of E(Fq): y^2 = x^3 + 4, almost surely outside G1"""
    x = int.from_bytes(hashlib.sha256(b"x%d" % seed).digest(), "big") % P.Q
    while True:
        rhs = (x * x * x + 4) % P.Q
        y = pow(rhs, (P.Q + 1) // 4, P.Q)
        if y * y % P.Q == rhs:
            return x.to_bytes(48, "big") + y.to_bytes(48, "big")
        x += 1


def test_ladder_parity(eng):
    from gpu_common import rand_g1
    xs = P.XORShift(77)
    pts = [rand_g1(xs) for _ in range(6)] + [_off_subgroup_g1(i) for i in range(6)] + [RC.hash_g1(b"h%d" % i) for i in range(2)]
    rnd = random.Random(3)
    ks = EDGE + [0, 3, 15, 16, (1 << 64) - 2] + [rnd.randrange(1 << 64) for _ in range(4)]
    A, B, want = [], [], []
    for i, p in enumerate(pts):
        for k in ks:
            A.append(np.frombuffer(g1_to_jac(p, rnd.randrange(1, P.Q)), np.uint64))
            b = np.zeros(18, np.uint64); b[0] = k
            B.append(b)
            want.append(RC.g1_mul(p, int(k).to_bytes(32, "big")))
    out, _ = eng.debug_op("G1_MUL_U64", np.stack(A), np.stack(B))
    for i in range(len(A)):
        assert RC.g1_jac_to_affine_bytes(out[i]) == want[i], i


# ---- 6. arguments, infinity ----------------------------------------------------------------------------------------------------------
def test_arguments_and_infinity(eng):
    from bls_amd import _native
    lib = _native.load()
    kind, n = "g2pubs", 32
    msgs, pks, sigs = _batch(eng, kind, n, seed=19)
    r = [5] * n; r[9] = 0
    with pytest.raises(Exception) as ei:
        rlc(eng, kind, msgs, pks, sigs, scalars=r)
    assert "-3" in str(ei.value) or "E_ARG" in str(ei.value)
    buf = (ctypes.c_uint8 * 1)(); off = (ctypes.c_uint64 * 1)(0); comb = ctypes.c_int(7)
    assert lib.blsmi_g2pubs_verify_batch_rlc(buf, off, buf, buf, None, None, None, None, ctypes.c_size_t(0), ctypes.byref(comb)) == 0 and comb.value == 0
    sc = (ctypes.c_uint64 * 1)(0)
    assert lib.blsmi_g1pubs_verify_batch_rlc(buf, off, buf, buf, None, sc, None, None, ctypes.c_size_t(1), None) == -3
    for k in KINDS:
        msgs, pks, sigs = _batch(eng, k, n, seed=21)
        inf = np.zeros(n, np.uint8); inf[3] = 1; inf[17] = 2
        ok, _, comb = rlc(eng, k, msgs, pks, sigs, inf=inf)
        assert comb == 0 and ok == vb(eng, k, msgs, pks, sigs, inf) and not ok[3] and not ok[17] and sum(ok) == n - 2
        p = pks.copy(); p[4] = 0                                                  # the all-zero record is infinity
        ok, _, comb = rlc(eng, k, msgs, p, sigs)
        assert comb == 0 and not ok[4] and sum(ok) == n - 1
        pj, sj = _jac_forms(k, pks, sigs, 1)
        sjb = bytearray(sj); w = 144 if k == "g2pubs" else 288
        z = (g1_to_jac(None) if k == "g2pubs" else g2_to_jac(None))
        sjb[w * 6:w * 7] = z                                                      # z = 0: infinity in the in-memory form
        okj, combj = rlc_jac(eng, k, msgs, pj, bytes(sjb))
        assert combj == 0 and not okj[6] and sum(okj) == n - 1


# ---- 7. the design size -----------------------------------------------------------------------------------------------------------------
def _profile(lib):
    buf = ctypes.create_string_buffer(1 << 16)
    lib.blsmi_last_profile(buf, ctypes.c_size_t(1 << 16))
    return buf.value.decode()


@pytest.mark.parametrize("kind,n", [("g2pubs", 65536), ("g1pubs", 16384)])
def test_design_size(eng, kind, n):
    from bls_amd import _native
    lib = _native.load()
    msgs, pks, sigs = _batch(eng, kind, n, seed=23)
    lib.blsmi_set_profiling(1)
    try:
        _profile(lib)
        ok, _, comb = rlc(eng, kind, msgs, pks, sigs)
        prof = _profile(lib)
    finally:
        lib.blsmi_set_profiling(0)
    assert comb == 1 and all(ok)
    for name in ("k_g1_mul_u64", "k_lat:aggtail2", "k_lat:miller1rawn", "k_g1_msm_bucket" if kind == "g2pubs" else "k_g2_msm_bucket"):
        assert name in prof, (name, prof[:2000])                                  # (G2: k_g2_msm_bucket or its lane-pair form)
    if kind == "g2pubs":
        assert "k_lat:powc12raw=" in prof                                         # the cofactor-power route
    bad = {5, n // 2, n - 1}
    m = list(msgs); m[5] = b"forged"
    s = sigs.copy(); s[n // 2] = sigs[0]
    p = pks.copy(); p[n - 1] = pks[1]
    ok, _, comb = rlc(eng, kind, m, p, s)
    assert comb == 0
    assert ok == vb(eng, kind, m, p, s)
    rnd = random.Random(1)
    for i in sorted(bad) + rnd.sample([i for i in range(n) if i not in bad], 16):
        assert ok[i] == oracle_verify(kind, m[i], p[i], s[i]) == (i not in bad), i


# ---- 8. split calls: one combined check per shard ----------------------------------------------------------------------------------
def test_split_call_per_shard(eng):
    env = dict(os.environ)
    env["BLSMI_DEVICE_ALIAS"] = "0,0"
    env["BLSMI_SHARD_MIN"] = "128"
    env["BLSMI_RLC_MIN"] = "0"
    env.pop("BLSMI_SHARDS", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rlc_alias_worker.py")], env=env, capture_output=True, text=True, timeout=600)
    line = [l for l in r.stdout.splitlines() if l.startswith("RLC_ALIAS ")]
    assert r.returncode == 0 and line, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert line[-1] == "RLC_ALIAS ok", line[-1]


# ---- 9. concurrency -----------------------------------------------------------------------------------------------------------------------
def test_concurrent_mixed_calls(eng):
    pool = {k: _batch(eng, k, 600, seed=29) for k in ("g2pubs", "g1pubs")}
    errors = []

    def worker(tid):
        rnd = random.Random(tid)
        try:
            for it in range(6):
                k = rnd.choice(("g2pubs", "g1pubs"))
                msgs, pks, sigs = pool[k]
                n = rnd.randrange(1, 300); lo = rnd.randrange(0, 600 - n)
                m = list(msgs[lo:lo + n]); p = pks[lo:lo + n].copy(); s = sigs[lo:lo + n].copy()
                bad = set(rnd.sample(range(n), rnd.randrange(0, min(3, n) + 1))) if rnd.random() < 0.5 else set()
                for i in bad:
                    m[i] = m[i] + b"!"
                want = [i not in bad for i in range(n)]
                if rnd.random() < 0.5:
                    ok, _, comb = rlc(eng, k, m, p, s)
                    if comb != (0 if bad else 1):
                        errors.append((tid, it, "combined", comb, sorted(bad)))
                else:
                    ok = vb(eng, k, m, p, s)
                if ok != want:
                    errors.append((tid, it, k, n, sorted(bad)))
        except Exception as e:                                                   # noqa: BLE001
            errors.append((tid, repr(e)))
    th = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors[:5]
