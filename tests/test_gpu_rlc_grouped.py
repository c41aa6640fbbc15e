"""-m gpu: grouped randomised batch verification (blsmi 0.11, blsmi_g?pubs_*verify*_batch_rlc_grouped[_jac]) and the weighted segmented
sums under it (blsmi_g?_sum_segmented_u64).  Tuple i is (table[msg_idx[i]], pk_i, sig_i); the tuples of one message share one pairing of
the combined check.  Expectations come from the oracle: sums of multiples (g?_sum of g?_mul), verify, and -- for the equation itself --
tests/test_rlc_grouped_cpu.py: grouped_holds."""
import ctypes
import hashlib
import random
import threading

import numpy as np
import pytest

from gpu_common import P, RC, rand_g1, rand_g2
from test_gpu_rlc import (DOMAIN, KINDS, _default_rlc_min, _jac_forms, _neg, _profile, _rand_sig_point, _sig_add, _sig_mul, _sks, oracle_verify, rlc, vb)

pytestmark = pytest.mark.gpu
EDGE = [1, 1 << 63, (1 << 64) - 1, 2]


@pytest.fixture(scope="module")
def eng():
    from bls_amd import engine
    engine.init(0)
    return engine                                                                # "rlc_min" stays at the header's default: it does not apply here


def _table(kind, d, seed):
    if kind == "domain":
        return [hashlib.sha256(b"grp-m-%d-%d" % (seed, j)).digest() for j in range(d)]
    return [b"grouped message %d/%d" % (seed, j) + b"y" * (j % 5) for j in range(d)]


def _gbatch(eng, kind, n, d, seed=0, msg_idx=None):
    """(table of d messages, msg_idx (n), pks (n, pkb), sigs (n, sgb)) of n valid tuples, signed on the device"""
    sks = _sks(n, seed + 1000)
    table = _table(kind, d, seed)
    if msg_idx is None:
        msg_idx = [i % d for i in range(n)]
    msgs = [table[j] for j in msg_idx]
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
    return table, list(msg_idx), np.asarray(pks, np.uint8).reshape(n, pkb).copy(), np.asarray(sigs, np.uint8).reshape(n, sgb).copy()


def grouped(eng, kind, table, msg_idx, pks, sigs, inf=None, scalars=None):
    """-> (ok list, combined)"""
    p, s = np.asarray(pks).tobytes(), np.asarray(sigs).tobytes()
    if kind == "domain":
        ok, bm, comb = eng.g1pubs_verify_with_domain_batch_rlc_grouped(table, DOMAIN, msg_idx, p, s, inf, scalars)
    else:
        fn = eng.g2pubs_verify_batch_rlc_grouped if kind == "g2pubs" else eng.g1pubs_verify_batch_rlc_grouped
        ok, bm, comb = fn(table, msg_idx, p, s, inf, scalars)
    assert np.array_equal(bm, np.packbits(np.asarray(ok, np.uint8), bitorder="little")[:len(bm)])
    return [bool(x) for x in ok], comb


def grouped_jac(eng, kind, table, msg_idx, pj, sj, scalars=None):
    if kind == "domain":
        ok, _, comb = eng.g1pubs_verify_with_domain_batch_rlc_grouped_jac(table, DOMAIN, msg_idx, pj, sj, scalars)
    else:
        fn = eng.g2pubs_verify_batch_rlc_grouped_jac if kind == "g2pubs" else eng.g1pubs_verify_batch_rlc_grouped_jac
        ok, _, comb = fn(table, msg_idx, pj, sj, scalars)
    return [bool(x) for x in ok], comb


def expand(table, msg_idx):
    return [table[j] for j in msg_idx]


# ---- 1. the weighted segmented sums, bit for bit ---------------------------------------------------------------------------------------
def _neg_point(group, pt):
    b = bytearray(pt)
    for o in ((48,) if group == 1 else (96, 144)):
        b[o:o + 48] = ((P.Q - int.from_bytes(b[o:o + 48], "big")) % P.Q).to_bytes(48, "big")
    return bytes(b)


@pytest.fixture(scope="module")
def weighted_cases():
    """per group: (pts, in_inf, scalars, idx, seg_off, want bytes, want inf) -- the oracle's answer, computed once"""
    out = {}
    for group in (1, 2):
        pb = 96 if group == 1 else 192
        xs = P.XORShift(400 + group)
        rnd = random.Random(group)
        pts = [(rand_g1 if group == 1 else rand_g2)(xs) for _ in range(48)]
        pts[11] = _neg_point(group, pts[10])
        r = EDGE + [rnd.randrange(1, 1 << 64) for _ in range(44)]
        r[11] = r[10]                                                            # P and -P with equal scalars
        r[13] = 0                                                                # a zero scalar
        in_inf = np.zeros(48, np.uint8); in_inf[12] = 1
        segs = [[], [5], [7, 7], [10, 11], [12, 3, 14], [13, 2, 0, 1], [12], [13],
                [rnd.randrange(48) for _ in range(65)], [rnd.randrange(48) for _ in range(130)]]
        mul = RC.g1_mul if group == 1 else RC.g2_mul
        add = RC.g1_sum if group == 1 else RC.g2_sum
        prod = {i: mul(pts[i], r[i].to_bytes(32, "big")) for i in range(48) if r[i] and not in_inf[i]}
        want, winf = b"", []
        for j, seg in enumerate(segs):
            parts = [prod[i] for i in seg if i in prod]
            if not parts or j == 3:
                want += bytes(pb); winf.append(1)
            else:
                want += add(b"".join(parts), len(parts)); winf.append(0)
        idx = [i for seg in segs for i in seg]
        off = np.cumsum([0] + [len(s) for s in segs]).astype(np.uint64)
        out[group] = (b"".join(pts), in_inf, r, idx, off, want, winf)
    return out


@pytest.mark.parametrize("group", (1, 2))
def test_weighted_sums_bit_for_bit(eng, weighted_cases, group):
    """empty, one point, the same index twice (jac_add's doubling case), P and -P, in_inf, a zero scalar, lengths 65 and 130; scalars 1, 2,
    2^63, 2^64 - 1; at segsum_chunk 0, 2 and 1024 the same bytes"""
    pts, in_inf, r, idx, off, want, winf = weighted_cases[group]
    fn = eng.g1_sum_segmented_u64 if group == 1 else eng.g2_sum_segmented_u64
    pb = 96 if group == 1 else 192
    try:
        for K in (0, 2, 1024):
            eng.set_option("segsum_chunk", K)
            got, ginf = fn(pts, 48, r, idx, off, in_inf)
            assert ginf.tolist() == winf, (group, K)
            for j in range(len(winf)):
                assert got[pb * j:pb * (j + 1)] == want[pb * j:pb * (j + 1)], (group, K, j)
    finally:
        eng.set_option("segsum_chunk", 0)
    # idx NULL: the positions themselves
    got, ginf = fn(pts, 48, r, None, [0, 2, 2, 10])
    mul = RC.g1_mul if group == 1 else RC.g2_mul
    add = RC.g1_sum if group == 1 else RC.g2_sum
    assert ginf.tolist() == [0, 1, 0]
    assert got[:pb] == add(b"".join(mul(pts[pb * i:pb * (i + 1)], r[i].to_bytes(32, "big")) for i in (0, 1)), 2)


# ---- 2. all valid ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_all_valid(eng, kind):
    for n in (1, 3, 64, 1000):
        for d in sorted({1, min(3, n), n}):
            table, idx, pks, sigs = _gbatch(eng, kind, n, d, seed=n + d)
            ok, comb = grouped(eng, kind, table, idx, pks, sigs)
            assert comb == 1 and all(ok) and len(ok) == n, (kind, n, d)
            if n <= 64:
                pj, sj = _jac_forms(kind, pks, sigs, n)
                okj, combj = grouped_jac(eng, kind, table, idx, pj, sj)
                assert combj == 1 and all(okj), (kind, n, d, "in-memory")
    # an entry nobody refers to (not a message at all for with_domain's 32-byte table: any bytes), and two entries with equal bytes
    table, idx, pks, sigs = _gbatch(eng, kind, 20, 3, seed=5, msg_idx=[0, 2] * 10)
    ok, comb = grouped(eng, kind, table, idx, pks, sigs)
    assert comb == 1 and all(ok)
    t2 = [table[0], table[1], table[2], table[0]]
    idx2 = [3 if (j == 0 and i % 4 == 0) else j for i, j in enumerate(idx)]
    ok, comb = grouped(eng, kind, t2, idx2, pks, sigs)
    assert comb == 1 and all(ok)


# ---- 3. "rlc_min" does not apply ---------------------------------------------------------------------------------------------------------
def test_rlc_min_does_not_apply(eng):
    from bls_amd import _native
    lib = _native.load()
    kind, n, d = "g1pubs", 64, 4
    table, idx, pks, sigs = _gbatch(eng, kind, n, d, seed=31)
    eng.set_option("rlc_min", _default_rlc_min())
    assert n < _default_rlc_min()
    assert rlc(eng, kind, expand(table, idx), pks, sigs)[2] == 0                 # the plain form, below the default rlc_min: per tuple
    lib.blsmi_set_profiling(1)
    try:
        _profile(lib)
        ok, comb = grouped(eng, kind, table, idx, pks, sigs)
        prof = _profile(lib)
    finally:
        lib.blsmi_set_profiling(0)
    assert comb == 1 and all(ok)
    assert "k_g1_segsum_chunk_u64" in prof, prof[:2000]
    table, idx, pks, sigs = _gbatch(eng, "g2pubs", n, d, seed=32)
    lib.blsmi_set_profiling(1)
    try:
        _profile(lib)
        ok, comb = grouped(eng, "g2pubs", table, idx, pks, sigs)
        prof = _profile(lib)
    finally:
        lib.blsmi_set_profiling(0)
    assert comb == 1 and all(ok) and "k_g2_segsum_chunk_u64" in prof, prof[:2000]


# ---- 4. the weights are per tuple inside a group -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_weights_are_per_tuple_inside_a_group(eng, kind):
    n, d = 12, 3
    idx = [i % d for i in range(n)]
    table, idx, pks, sigs = _gbatch(eng, kind, n, d, seed=41, msg_idx=idx)
    a, b = 3, 9                                                                  # both of message 0
    s = sigs.copy(); s[[a, b]] = sigs[[b, a]]
    rnd = random.Random(6)
    r = [rnd.randrange(1, 1 << 64) for _ in range(n)]
    req = list(r); req[b] = req[a]
    ok, comb = grouped(eng, kind, table, idx, pks, s, scalars=req)
    assert comb == 1 and all(ok)                                                 # r_a == r_b: unnoticed, the documented caller responsibility
    msgs = expand(table, idx)
    for sc in (r, None):                                                         # r_a != r_b, and drawn scalars
        ok, comb = grouped(eng, kind, table, idx, pks, s, scalars=sc)
        assert comb == 0 and [i for i in range(n) if not ok[i]] == [a, b], (kind, sc is None)
        for i in (a, b, 0):
            assert ok[i] == oracle_verify(kind, msgs[i], pks[i], s[i])


@pytest.mark.parametrize("kind", KINDS)
def test_caller_scalars_applied_exactly_across_groups(eng, kind):
    """sig_a += r_b D, sig_b -= r_a D with a and b in DIFFERENT groups: the signature sum is unchanged exactly when the scalars are r"""
    n, d = 8, 2
    table, idx, pks, sigs = _gbatch(eng, kind, n, d, seed=43, msg_idx=[0, 1, 0, 1, 1, 0, 1, 0])
    rnd = random.Random(5)
    r = EDGE + [rnd.randrange(1, 1 << 64) for _ in range(n - len(EDGE))]
    a, b = 2, 1                                                                  # r_a = 2^64 - 1 (message 0), r_b = 2^63 (message 1)
    D = _rand_sig_point(kind, 4)
    s = sigs.copy()
    s[a] = np.frombuffer(_sig_add(kind, sigs[a], _sig_mul(kind, D, r[b])), np.uint8)
    s[b] = np.frombuffer(_sig_add(kind, sigs[b], _neg(kind, _sig_mul(kind, D, r[a]))), np.uint8)
    ok, comb = grouped(eng, kind, table, idx, pks, s, scalars=r)
    assert comb == 1 and all(ok)
    ok, comb = grouped(eng, kind, table, idx, pks, s)
    assert comb == 0 and not ok[a] and not ok[b] and sum(ok) == n - 2
    r3 = list(r); r3[a] = r[a] - 1
    assert grouped(eng, kind, table, idx, pks, s, scalars=r3)[1] == 0


# ---- 5. the grouping is honoured ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_grouping_is_honoured(eng, kind):
    n, d = 24, 4
    table, idx, pks, sigs = _gbatch(eng, kind, n, d, seed=47)
    bad = 7
    idx2 = list(idx); idx2[bad] = (idx[bad] + 1) % d
    ok, comb = grouped(eng, kind, table, idx2, pks, sigs)
    msgs = expand(table, idx2)
    assert comb == 0 and [i for i in range(n) if not ok[i]] == [bad]
    assert ok == vb(eng, kind, msgs, pks, sigs)
    for i in (bad, 0, n - 1):
        assert ok[i] == oracle_verify(kind, msgs[i], pks[i], sigs[i])


# ---- 6. fallbacks -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_fallbacks_give_verify_batch_verdicts(eng, kind):
    from gpu_common import g1_to_jac, g2_to_jac
    n, d = 32, 5
    table, idx, pks, sigs = _gbatch(eng, kind, n, d, seed=53)
    msgs = expand(table, idx)
    p = pks.copy(); p[9] = pks[10]
    ok, comb = grouped(eng, kind, table, idx, p, sigs)                           # a wrong key
    assert comb == 0 and ok == vb(eng, kind, msgs, p, sigs) and not ok[9] and sum(ok) == n - 1
    s = sigs.copy(); s[20] = np.frombuffer(_rand_sig_point(kind, 1), np.uint8)
    ok, comb = grouped(eng, kind, table, idx, pks, s)                            # a tampered signature
    assert comb == 0 and ok == vb(eng, kind, msgs, pks, s) and not ok[20] and sum(ok) == n - 1
    inf = np.zeros(n, np.uint8); inf[3] = 1; inf[17] = 2
    ok, comb = grouped(eng, kind, table, idx, pks, sigs, inf=inf)                # inf_flags bits 0 and 1
    assert comb == 0 and ok == vb(eng, kind, msgs, pks, sigs, inf) and not ok[3] and not ok[17] and sum(ok) == n - 2
    p = pks.copy(); p[4] = 0
    ok, comb = grouped(eng, kind, table, idx, p, sigs)                           # the all-zero record
    assert comb == 0 and ok == vb(eng, kind, msgs, p, sigs) and not ok[4] and sum(ok) == n - 1
    pj, sj = _jac_forms(kind, pks, sigs, 1)
    sjb = bytearray(sj); w = 144 if kind == "g2pubs" else 288
    sjb[w * 6:w * 7] = g1_to_jac(None) if kind == "g2pubs" else g2_to_jac(None)   # z = 0 in the in-memory form
    okj, combj = grouped_jac(eng, kind, table, idx, pj, bytes(sjb))
    if kind == "domain":
        want = [bool(x) for x in eng.g1pubs_verify_with_domain_batch_jac(msgs, DOMAIN, pj, bytes(sjb))]
    else:
        want = [bool(x) for x in (eng.g2pubs_verify_batch_jac if kind == "g2pubs" else eng.g1pubs_verify_batch_jac)(msgs, pj, bytes(sjb))[0]]
    assert combj == 0 and okj == want and not okj[6] and sum(okj) == n - 1


def test_group_sum_at_infinity_falls_back(eng):
    """pk_b = -pk_a in one group with r_a == r_b: the group's weighted sum is infinity, the call takes the per-tuple path"""
    kind, n, d = "g1pubs", 6, 2
    table, idx, pks, sigs = _gbatch(eng, kind, n, d, seed=59, msg_idx=[0, 1, 0, 1, 1, 1])             # group 0 = {0, 2}
    p = pks.copy(); p[2] = np.frombuffer(_neg_point(1, bytes(pks[0])), np.uint8)
    r = [9, 5, 9, 6, 7, 8]
    ok, comb = grouped(eng, kind, table, idx, p, sigs, scalars=r)
    assert comb == 0 and ok == vb(eng, kind, expand(table, idx), p, sigs) and not ok[2] and sum(ok) == n - 1


# ---- 7. arguments -------------------------------------------------------------------------------------------------------------------------
def test_arguments(eng):
    from bls_amd import _native
    lib = _native.load()
    kind, n, d = "g2pubs", 16, 2
    table, idx, pks, sigs = _gbatch(eng, kind, n, d, seed=61)
    for t, ix, sc in ((table, [d] + idx[1:], None), (table, idx, [5] * 9 + [0] + [5] * 6), ([], idx, None)):   # an index >= d, a zero scalar, d = 0 with n > 0
        with pytest.raises(eng.BlsmiError) as ei:
            grouped(eng, kind, t, ix, pks, sigs, scalars=sc)
        assert "(-3)" in str(ei.value)                                           # BLSMI_E_ARG
    buf = (ctypes.c_uint8 * 1)(); off = (ctypes.c_uint64 * 1)(0); comb = ctypes.c_int(7)
    assert lib.blsmi_g2pubs_verify_batch_rlc_grouped(buf, off, ctypes.c_size_t(0), None, buf, buf, None, None, None, None, ctypes.c_size_t(0), ctypes.byref(comb)) == 0
    assert comb.value == 0


# ---- 8. a filled shape ----------------------------------------------------------------------------------------------------------------
def test_filled_shape(eng):
    from bls_amd import _native
    lib = _native.load()
    kind, n, d = "g1pubs", 8192, 64
    table, idx, pks, sigs = _gbatch(eng, kind, n, d, seed=67)
    lib.blsmi_set_profiling(1)
    try:
        _profile(lib)
        ok, comb = grouped(eng, kind, table, idx, pks, sigs)
        prof = _profile(lib)
    finally:
        lib.blsmi_set_profiling(0)
    assert comb == 1 and all(ok)
    for name in ("k_g1_segsum_chunk_u64", "k_g2_msm_bucket", "k_lat:aggtail2"):
        assert name in prof, (name, prof[:2000])
    bad = {5, n // 2, n - 1}
    idx2 = list(idx); idx2[5] = (idx[5] + 1) % d
    s = sigs.copy(); s[n // 2] = sigs[0]
    p = pks.copy(); p[n - 1] = pks[1]
    ok, comb = grouped(eng, kind, table, idx2, p, s)
    msgs = expand(table, idx2)
    assert comb == 0
    assert ok == vb(eng, kind, msgs, p, s)
    rnd = random.Random(1)
    for i in sorted(bad) + rnd.sample([i for i in range(n) if i not in bad], 16):
        assert ok[i] == oracle_verify(kind, msgs[i], p[i], s[i]) == (i not in bad), i


# ---- 9. concurrency -------------------------------------------------------------------------------------------------------------------
def test_concurrent_mixed_calls(eng):
    d = 7
    pool = {k: _gbatch(eng, k, 600, d, seed=71) for k in ("g2pubs", "g1pubs")}
    errors = []

    def worker(tid):
        rnd = random.Random(tid)
        try:
            for it in range(6):
                k = rnd.choice(("g2pubs", "g1pubs"))
                table, idx, pks, sigs = pool[k]
                n = rnd.randrange(1, 300); lo = rnd.randrange(0, 600 - n)
                ix = list(idx[lo:lo + n]); p = pks[lo:lo + n].copy(); s = sigs[lo:lo + n].copy()
                bad = set(rnd.sample(range(n), rnd.randrange(0, min(3, n) + 1))) if rnd.random() < 0.5 else set()
                for i in bad:
                    ix[i] = (ix[i] + 1 + rnd.randrange(d - 1)) % d
                want = [i not in bad for i in range(n)]
                which = rnd.randrange(3)
                if which == 0:
                    ok, comb = grouped(eng, k, table, ix, p, s)
                    if comb != (0 if bad else 1):
                        errors.append((tid, it, "combined", comb, sorted(bad)))
                elif which == 1:
                    ok = rlc(eng, k, expand(table, ix), p, s)[0]
                else:
                    ok = vb(eng, k, expand(table, ix), p, s)
                if ok != want:
                    errors.append((tid, it, k, n, which, sorted(bad)))
        except Exception as e:                                                   # noqa: BLE001
            errors.append((tid, repr(e)))
    th = [threading.Thread(target=worker, args=(t,)) for t in range(6)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors[:5]
