"""-m gpu: randomised batch verification that finds the bad tuples by blocks (blsmi 0.12, blsmi_g?pubs_*verify*_batch_rlc_locate[_jac]).
The total check is that of *_verify_batch_rlc; when it fails, one pairing equation per block of `block` tuples decides which blocks hold,
and only the tuples of the others get verify_batch's verdicts.  Cases run at n = 70 / 71 with block = 8 unless said otherwise: a ragged
last block of 6 (7) tuples, an odd record count, the latency layouts.  The expected per-block verdicts are composed from the oracle: 64-bit
multiples, the block's signature sum, one Miller loop over its pair list, the final exponentiation."""
import ctypes
import hashlib
import os
import random
import re
import threading

import numpy as np
import pytest

from gpu_common import P, RC, g1_to_jac, g2_to_jac

pytestmark = pytest.mark.gpu
KINDS = ("g2pubs", "g1pubs", "domain")
DOMAIN = bytes(range(1, 9))
N, BLOCK = 70, 8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _default_rlc_min():
    return int(re.search(r'"rlc_min" \(BLSMI_RLC_MIN, default (\d+)\)', open(os.path.join(ROOT, "include", "blsmi.h")).read()).group(1))


@pytest.fixture(scope="module")
def eng():
    from bls_amd import engine
    engine.init(0)
    return engine


def _sks(n, seed):
    return b"".join(hashlib.sha256(b"loc-sk-%d-%d" % (seed, i)).digest()[:31].rjust(32, b"\0") for i in range(n))


def _msgs(kind, n, seed):
    if kind == "domain":
        return [hashlib.sha256(b"loc-m-%d-%d" % (seed, i)).digest() for i in range(n)]
    return [b"locate message %d/%d" % (seed, i) + b"x" * (i % 7) for i in range(n)]


_BATCHES = {}


def _batch(eng, kind, n, seed=0):
    """(msgs, pks (n, pkb), sigs (n, sgb)) of n valid tuples, signed on the device once per (kind, n, seed); callers copy before they change"""
    key = (kind, n, seed)
    if key not in _BATCHES:
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
        _BATCHES[key] = (msgs, np.asarray(pks, np.uint8).reshape(n, pkb).copy(), np.asarray(sigs, np.uint8).reshape(n, sgb).copy())
    msgs, pks, sigs = _BATCHES[key]
    return list(msgs), pks.copy(), sigs.copy()


def locate(eng, kind, msgs, pks, sigs, inf=None, scalars=None, block=BLOCK):
    """-> (ok list, combined, rechecked)"""
    p, s = np.asarray(pks).tobytes(), np.asarray(sigs).tobytes()
    if kind == "domain":
        ok, bm, comb, re_ = eng.g1pubs_verify_with_domain_batch_rlc_locate(msgs, DOMAIN, p, s, inf, scalars, block)
    else:
        fn = eng.g2pubs_verify_batch_rlc_locate if kind == "g2pubs" else eng.g1pubs_verify_batch_rlc_locate
        ok, bm, comb, re_ = fn(msgs, p, s, inf, scalars, block)
    assert np.array_equal(bm, np.packbits(np.asarray(ok, np.uint8), bitorder="little")[:len(bm)])
    return [bool(x) for x in ok], comb, re_


def locate_jac(eng, kind, msgs, pj, sj, scalars=None, block=BLOCK):
    if kind == "domain":
        ok, _, comb, re_ = eng.g1pubs_verify_with_domain_batch_rlc_locate_jac(msgs, DOMAIN, pj, sj, scalars, block)
    else:
        fn = eng.g2pubs_verify_batch_rlc_locate_jac if kind == "g2pubs" else eng.g1pubs_verify_batch_rlc_locate_jac
        ok, _, comb, re_ = fn(msgs, pj, sj, scalars, block)
    return [bool(x) for x in ok], comb, re_


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


def _fe(f):
    return RC.final_exponentiation(f)[1]


def oracle_block(kind, msgs, pks, sigs, r, lo, hi):
    """the equation of the block of tuples lo .. hi - 1 with scalars r, composed from the oracle's primitives"""
    idx = range(lo, hi)
    k32 = {i: int(r[i]).to_bytes(32, "big") for i in idx}
    if kind == "g2pubs":
        S = RC.g1_sum(b"".join(RC.g1_mul(bytes(sigs[i]), k32[i]) for i in idx), hi - lo)
        lhs = _fe(RC.miller_loop(S, RC.g2_generator(), 1))
        rhs = _fe(RC.miller_loop(b"".join(RC.g1_mul(RC.hash_g1(msgs[i]), k32[i]) for i in idx), b"".join(bytes(pks[i]) for i in idx), hi - lo))
    else:
        S = RC.g2_sum(b"".join(RC.g2_mul(bytes(sigs[i]), k32[i]) for i in idx), hi - lo)
        lhs = _fe(RC.miller_loop(RC.g1_generator(), S, 1))
        H = b"".join(RC.hash_g2(msgs[i]) if kind == "g1pubs" else RC.hash_g2_with_domain(msgs[i], DOMAIN) for i in idx)
        rhs = _fe(RC.miller_loop(b"".join(RC.g1_mul(bytes(pks[i]), k32[i]) for i in idx), H, hi - lo))
    return bool(np.array_equal(lhs, rhs))


def _blocks(n, block):
    return [(lo, min(n, lo + block)) for lo in range(0, n, block)]


def _sizes_of_blocks_with(n, block, bad):
    return sum(hi - lo for lo, hi in _blocks(n, block) if any(lo <= i < hi for i in bad))


def _neg(kind, pt):
    b = bytearray(pt)
    for o in ((48,) if kind == "g2pubs" else (96, 144)):
        y = int.from_bytes(b[o:o + 48], "big")
        b[o:o + 48] = ((P.Q - y) % P.Q).to_bytes(48, "big")
    return bytes(b)


def _sig_add(kind, a, b):
    return (RC.g1_sum if kind == "g2pubs" else RC.g2_sum)(bytes(a) + bytes(b), 2)


def _rand_sig_point(kind, seed):
    k = hashlib.sha256(b"locD%d" % seed).digest()[:31].rjust(32, b"\0")
    return RC.g1_mul(RC.g1_generator(), k) if kind == "g2pubs" else RC.g2_mul(RC.g2_generator(), k)


def _other(kind, m):
    return hashlib.sha256(b"other" + m).digest() if kind == "domain" else m + b"!"


def _jac_forms(kind, pks, sigs, seed):
    rnd = random.Random(seed)
    if kind == "g2pubs":
        pj = [g2_to_jac(bytes(p), (rnd.randrange(1, P.Q), rnd.randrange(P.Q))) for p in pks]
        sj = [g1_to_jac(bytes(s), rnd.randrange(1, P.Q)) for s in sigs]
    else:
        pj = [g1_to_jac(bytes(p), rnd.randrange(1, P.Q)) for p in pks]
        sj = [g2_to_jac(bytes(s), (rnd.randrange(1, P.Q), rnd.randrange(P.Q))) for s in sigs]
    return pj, sj


def _profile(lib):
    buf = ctypes.create_string_buffer(1 << 16)
    lib.blsmi_last_profile(buf, ctypes.c_size_t(1 << 16))
    names = [seg.split("=")[0] for seg in buf.value.decode().split(";") if seg]
    return [x for x in names if x != "(between)"]                                 # (the time between two marked stretches: not a kernel)


# ---- 1. all valid ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_all_valid_affine_and_in_memory(eng, kind):
    for n in (N, N + 1):
        msgs, pks, sigs = _batch(eng, kind, n)
        ok, comb, re_ = locate(eng, kind, msgs, pks, sigs)
        assert all(ok) and len(ok) == n and comb == 1 and re_ == 0, (kind, n)
        pj, sj = _jac_forms(kind, pks, sigs, n)
        ok, comb, re_ = locate_jac(eng, kind, msgs, b"".join(pj), b"".join(sj))
        assert all(ok) and len(ok) == n and comb == 1 and re_ == 0, (kind, n, "in-memory")
    ok, comb, re_ = locate(eng, kind, msgs[:1], pks[:1], sigs[:1], block=0)       # one tuple, the automatic block
    assert ok == [True] and comb == 1 and re_ == 0


# ---- 2. corruptions ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_corruptions_recheck_their_blocks_only(eng, kind):
    msgs, pks, sigs = _batch(eng, kind, N)
    for block in (8, 2, 70, 1024):
        every = [lo for lo, _ in _blocks(N, block)]
        for bad in ({0, 7, 8, 69}, set(every), {17}):
            m = list(msgs); p = pks.copy(); s = sigs.copy()
            for j, i in enumerate(sorted(bad)):
                if j % 3 == 0:
                    m[i] = _other(kind, m[i])                                     # wrong message
                elif j % 3 == 1:
                    p[i] = pks[(i + 1) % N]                                       # wrong key
                else:
                    s[i] = np.frombuffer(_rand_sig_point(kind, i), np.uint8)      # tampered signature
            ok, comb, re_ = locate(eng, kind, m, p, s, block=block)
            assert comb == 0, (kind, block, sorted(bad))
            assert ok == vb(eng, kind, m, p, s) == [i not in bad for i in range(N)], (kind, block, sorted(bad))
            assert re_ == _sizes_of_blocks_with(N, block, bad), (kind, block, sorted(bad), re_)
            if block == 8 and len(bad) == 4:
                for i in sorted(bad):
                    assert oracle_verify(kind, m[i], p[i], s[i]) is False and oracle_verify(kind, msgs[i], pks[i], sigs[i]) is True, (kind, i)


# ---- 3. the block arithmetic, pinned by caller scalars ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_block_arithmetic_pinned_by_caller_scalars(eng, kind):
    n = N + 1
    msgs, pks, sigs = _batch(eng, kind, n)
    rnd = random.Random(31)
    r = [rnd.randrange(1, 1 << 64) for _ in range(n)]
    r[0], r[1], r[2] = 1, 1 << 63, (1 << 64) - 1
    a, c, w = 10, 43, 70                                                          # blocks 1, 5 and the ragged last one
    r[c] = r[a]
    D = _rand_sig_point(kind, 7)
    s = sigs.copy()
    s[a] = np.frombuffer(_sig_add(kind, sigs[a], D), np.uint8)
    s[c] = np.frombuffer(_sig_add(kind, sigs[c], _neg(kind, D)), np.uint8)
    m = list(msgs); m[w] = _other(kind, m[w])
    want_blocks = [oracle_block(kind, m, pks, s, r, lo, hi) for lo, hi in _blocks(n, BLOCK)]
    assert want_blocks == [b not in (1, 5, 8) for b in range(9)]
    ok, comb, re_ = locate(eng, kind, m, pks, s, scalars=r)
    assert comb == 0 and re_ == 8 + 8 + 7, (kind, comb, re_)
    assert ok == [i not in (a, c, w) for i in range(n)] == vb(eng, kind, m, pks, s)
    # without the wrong message the total holds under these scalars (r_a D - r_c D = 0), though two of its blocks would not: nothing is rechecked
    ok, comb, re_ = locate(eng, kind, msgs, pks, s, scalars=r)
    assert comb == 1 and all(ok) and re_ == 0
    ok, comb, re_ = locate(eng, kind, msgs, pks, s)                               # drawn scalars: caught, in two blocks
    assert comb == 0 and re_ == 16 and ok == [i not in (a, c) for i in range(n)]


@pytest.mark.parametrize("kind", ("g2pubs", "g1pubs"))
def test_same_pair_inside_one_block(eng, kind):
    msgs, pks, sigs = _batch(eng, kind, N)
    r = [3 + 2 * i for i in range(N)]
    a, c = 17, 22                                                                 # both in block 2
    r[c] = r[a]
    D = _rand_sig_point(kind, 9)
    s = sigs.copy()
    s[a] = np.frombuffer(_sig_add(kind, sigs[a], D), np.uint8)
    s[c] = np.frombuffer(_sig_add(kind, sigs[c], _neg(kind, D)), np.uint8)
    assert oracle_block(kind, msgs, pks, s, r, 16, 24)
    ok, comb, re_ = locate(eng, kind, msgs, pks, s, scalars=r)                    # the documented caveat of caller scalars
    assert comb == 1 and all(ok) and re_ == 0
    m = list(msgs); m[60] = _other(kind, m[60])                                   # the total fails elsewhere: block 2 still holds, as its equation does
    ok, comb, re_ = locate(eng, kind, m, pks, s, scalars=r)
    assert comb == 0 and re_ == 8 and ok == [i != 60 for i in range(N)]
    ok, comb, re_ = locate(eng, kind, msgs, pks, s)
    assert comb == 0 and re_ == 8 and ok == [i not in (a, c) for i in range(N)]


# ---- 4. infinity --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_infinity_fails_its_block_only(eng, kind):
    msgs, pks, sigs = _batch(eng, kind, N)
    for i, flag in ((12, 1), (69, 2)):                                            # a flagged key, a flagged signature (in the ragged block)
        inf = np.zeros(N, np.uint8); inf[i] = flag
        ok, comb, re_ = locate(eng, kind, msgs, pks, sigs, inf=inf)
        assert comb == 0 and ok == [j != i for j in range(N)] == vb(eng, kind, msgs, pks, sigs, inf), (kind, i)
        assert re_ == (8 if i < 64 else 6), (kind, i, re_)
    p = pks.copy(); p[33] = 0                                                     # the all-zero record
    ok, comb, re_ = locate(eng, kind, msgs, p, sigs)
    assert comb == 0 and re_ == 8 and ok == [j != 33 for j in range(N)]
    s = sigs.copy(); s[0] = 0
    ok, comb, re_ = locate(eng, kind, msgs, pks, s, block=2)
    assert comb == 0 and re_ == 2 and ok == [j != 0 for j in range(N)]
    pj, sj = _jac_forms(kind, pks, sigs, 3)
    sj[41] = g1_to_jac(None) if kind == "g2pubs" else g2_to_jac(None)             # z = 0
    ok, comb, re_ = locate_jac(eng, kind, msgs, b"".join(pj), b"".join(sj))
    assert comb == 0 and re_ == 8 and ok == [j != 41 for j in range(N)]


@pytest.mark.parametrize("kind", ("g2pubs", "g1pubs"))
def test_block_sum_at_infinity(eng, kind):
    msgs, pks, sigs = _batch(eng, kind, N)
    r = [5 + i for i in range(N)]
    r[21] = r[20]
    s = sigs.copy(); s[21] = np.frombuffer(_neg(kind, bytes(sigs[20])), np.uint8)  # r_20 sig_20 + r_21 (-sig_20) = 0: block 10 of block = 2
    ok, comb, re_ = locate(eng, kind, msgs, pks, s, scalars=r, block=2)
    assert comb == 0 and re_ == 2 and ok == [j != 21 for j in range(N)] == vb(eng, kind, msgs, pks, s)


# ---- 5. layouts ---------------------------------------------------------------------------------------------------------------------
def test_layouts_give_identical_results(eng):
    from bls_amd import _native
    lib = _native.load()
    n = N + 1
    settings = {"k_lat:miller1raw": lambda: None,
                "k_miller1s_row": lambda: eng.set_row_threshold(1, 1 << 20),
                "k_miller1x2_quad": lambda: (eng.set_row_threshold(0, 0), eng.set_latency_threshold(0)),
                "k_miller1x2_pair": lambda: (eng.set_row_threshold(0, 0), eng.set_latency_threshold(0), eng.set_quad_threshold(0))}
    fe_seen = set()
    for kind in ("g2pubs", "g1pubs"):
        msgs, pks, sigs = _batch(eng, kind, n)
        bad = {3, 40, 70}
        m = list(msgs)
        for i in bad:
            m[i] = _other(kind, m[i])
        for block in (8, 2):
            want_re = _sizes_of_blocks_with(n, block, bad)
            for name, apply in settings.items():
                try:
                    apply()
                    lib.blsmi_set_profiling(1)
                    _profile(lib)
                    ok, comb, re_ = locate(eng, kind, m, pks, sigs, block=block)
                    prof = _profile(lib)
                    okv, combv, rev = locate(eng, kind, msgs, pks, sigs, block=block)
                finally:
                    lib.blsmi_set_profiling(0)
                    eng.set_latency_threshold(8192); eng.set_quad_threshold(16384); eng.set_row_threshold(*eng.ROW_DEFAULT)
                assert name in prof and "k_fq12_seg_prod_row" in prof and "k_fq12_mul_pairs_row" in prof and "k_fq12_is_one_m384" in prof, (kind, block, name, prof)
                assert comb == 0 and re_ == want_re and ok == [i not in bad for i in range(n)], (kind, block, name, re_)
                assert combv == 1 and rev == 0 and all(okv), (kind, block, name)
                fe_seen |= set(prof) & {"k_lat:finalexp1", "k_final_exp_row", "k_final_exp_quad", "k_final_exp_pair"}
    assert {"k_lat:finalexp1", "k_final_exp_row"} <= fe_seen, fe_seen       # the block checks' final exponentiation: wave and row (and quad beyond)


def test_segsum_chunk_option(eng):
    kind = "g1pubs"
    msgs, pks, sigs = _batch(eng, kind, N)
    m = list(msgs); m[9] = _other(kind, m[9]); m[64] = _other(kind, m[64])
    got = []
    try:
        for k in (0, 2, 1024):
            eng.set_option("segsum_chunk", k)
            got.append(locate(eng, kind, m, pks, sigs))
    finally:
        eng.set_option("segsum_chunk", 0)
    assert got[0] == got[1] == got[2]
    assert got[0] == ([i not in (9, 64) for i in range(N)], 0, 8 + 6)


# ---- 6. the call that holds launches what _rlc launches ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("g2pubs", "g1pubs"))
def test_happy_path_against_rlc(eng, kind):
    from bls_amd import _native
    lib = _native.load()
    n = N + 1
    msgs, pks, sigs = _batch(eng, kind, n)
    p, s = pks.tobytes(), sigs.tobytes()
    r = [7 + i for i in range(n)]
    rlc_min = _default_rlc_min()
    try:
        eng.set_option("rlc_min", 0)
        lib.blsmi_set_profiling(1)
        _profile(lib)
        ok0, _, comb0 = (eng.g2pubs_verify_batch_rlc if kind == "g2pubs" else eng.g1pubs_verify_batch_rlc)(msgs, p, s, None, r)
        prof_rlc = _profile(lib)
        ok1, comb1, re1 = locate(eng, kind, msgs, pks, sigs, scalars=r)
        prof_loc = _profile(lib)
    finally:
        lib.blsmi_set_profiling(0)
        eng.set_option("rlc_min", rlc_min)
    assert comb0 == 1 and all(ok0) and comb1 == 1 and all(ok1) and re1 == 0
    tree = ("k_lat:mul12raw", "k_fq12_prod_level")
    assert prof_loc.count("k_fq12_seg_prod_row") == 1 and "k_fq12_seg_prod_row" not in prof_rlc
    assert [x for x in prof_loc if x not in tree and x != "k_fq12_seg_prod_row"] == [x for x in prof_rlc if x not in tree], (prof_loc, prof_rlc)
    levels = lambda prof: sum(prof.count(x) for x in tree)                        # noqa: E731
    assert 0 < levels(prof_loc) < levels(prof_rlc), (prof_loc, prof_rlc)          # 9 block values against 71 Miller values
    i = prof_loc.index("k_fq12_seg_prod_row")
    assert set(prof_loc[i + 1:i + 1 + levels(prof_loc)]) <= set(tree)             # the tree follows the block values
    assert prof_loc[-1] == "k_lat:aggtail2" and not [x for x in prof_loc if "final_exp" in x or "finalexp" in x]


# ---- 7. concurrency -------------------------------------------------------------------------------------------------------------------
def test_concurrent_mixed_calls(eng):
    pool = {k: _batch(eng, k, 320, seed=5) for k in ("g2pubs", "g1pubs")}
    rlc_min = _default_rlc_min()
    errors = []

    def worker(tid):
        rnd = random.Random(tid)
        try:
            for it in range(4):
                k = ("g2pubs", "g1pubs")[(tid + it) % 2]
                msgs, pks, sigs = pool[k]
                n = rnd.randrange(280, 320)
                m = list(msgs[:n]); p = pks[:n]; s = sigs[:n]
                bad = set(rnd.sample(range(n), rnd.randrange(1, 4))) if rnd.random() < 0.6 else set()
                for i in bad:
                    m[i] = m[i] + b"!"
                want = [i not in bad for i in range(n)]
                which = (tid + it) % 3
                if which == 0:
                    block = rnd.choice((0, 2, 8, 64))
                    ok, comb, re_ = locate(eng, k, m, p, s, block=block)
                    b = block or 64
                    if comb != (0 if bad else 1) or re_ != _sizes_of_blocks_with(n, b, bad):
                        errors.append((tid, it, "locate", comb, re_, sorted(bad)))
                elif which == 1:
                    fn = eng.g2pubs_verify_batch_rlc if k == "g2pubs" else eng.g1pubs_verify_batch_rlc
                    ok = [bool(x) for x in fn(m, p.tobytes(), s.tobytes())[0]]
                else:
                    ok = vb(eng, k, m, p, s)
                if ok != want:
                    errors.append((tid, it, k, n, which, sorted(bad)))
        except Exception as e:                                                   # noqa: BLE001
            errors.append((tid, repr(e)))
    try:
        eng.set_option("rlc_min", 0)
        th = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
        for t in th:
            t.start()
        for t in th:
            t.join()
    finally:
        eng.set_option("rlc_min", rlc_min)
    assert not errors, errors[:5]


# ---- 8. the design size ---------------------------------------------------------------------------------------------------------------
def test_design_size_one_bad_tuple(eng):
    kind, n = "g2pubs", 65536
    msgs, pks, sigs = _batch(eng, kind, n, seed=23)
    bad = 40000
    msgs[bad] = b"forged"
    ok, comb, re_ = locate(eng, kind, msgs, pks, sigs, block=0)
    assert comb == 0 and re_ == 256, (comb, re_)                                  # the automatic block at 65 536 tuples
    assert ok.count(False) == 1 and ok[bad] is False
    assert oracle_verify(kind, msgs[bad], pks[bad], sigs[bad]) is False
