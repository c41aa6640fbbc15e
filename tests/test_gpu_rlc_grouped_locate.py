"""-m gpu: grouped randomised batch verification that finds the bad tuples by cells (blsmi 0.13,
blsmi_g?pubs_*verify*_batch_rlc_grouped_locate[_jac]).  Tuple i is (table[msg_idx[i]], pk_i, sig_i); the tuples of every message are cut
into cells of at most `block` tuples, keys and signatures are summed per cell, and when the total check fails one pairing equation per cell
decides which tuples get verify_batch's verdicts.  The base shape: n = 70 / 71 over a table of 6 messages, one of them unreferenced, groups
of 1, 2, 9, 25 and 33 (34) tuples, interleaved so that the plan's permutation is no identity; block = 4 cuts them into cells of
1 / 2 / 4+4+1 / 6x4+1 / 8x4+1 (+2).  Expected cells come from the pure-Python mirror of the cut (tests/test_rlc_grouped_locate_cpu.py),
expected per-cell verdicts from the oracle: 64-bit multiples, the cell's two sums, a Miller loop a side, the final exponentiation."""
import random
import threading

import numpy as np
import pytest

from gpu_common import RC, g1_to_jac, g2_to_jac
from test_gpu_rlc_grouped import _gbatch, expand, grouped
from test_gpu_rlc_locate import (DOMAIN, KINDS, _default_rlc_min, _fe, _jac_forms, _neg, _profile, _rand_sig_point, _sig_add, locate, oracle_verify, vb)
from test_rlc_grouped_locate_cpu import cells_mirror

pytestmark = pytest.mark.gpu
N, BLOCK, D = 70, 4, 6
SIZES = {70: (1, 2, 0, 9, 25, 33), 71: (1, 2, 0, 9, 25, 34)}


@pytest.fixture(scope="module")
def eng():
    from bls_amd import engine
    engine.init(0)
    return engine                                                                # "rlc_min" stays at the header's default: it does not apply here


def _interleaved(sizes):
    """msg_idx with sizes[j] tuples of entry j, dealt round-robin from the last entry down"""
    left = list(sizes)
    out = []
    while any(left):
        for j in reversed(range(len(left))):
            if left[j]:
                out.append(j)
                left[j] -= 1
    return out


_BATCHES = {}


def _batch(eng, kind, n=N, sizes=None, seed=0):
    """(table, msg_idx, pks, sigs) of n valid tuples, signed on the device once per (kind, n); callers copy before they change"""
    key = (kind, n, seed)
    if key not in _BATCHES:
        sizes = sizes or SIZES[n]
        _BATCHES[key] = _gbatch(eng, kind, n, len(sizes), seed=seed + 40, msg_idx=_interleaved(sizes))
    table, idx, pks, sigs = _BATCHES[key]
    return list(table), list(idx), pks.copy(), sigs.copy()


def gl(eng, kind, table, msg_idx, pks, sigs, inf=None, scalars=None, block=BLOCK):
    """-> (ok list, combined, rechecked)"""
    p, s = np.asarray(pks).tobytes(), np.asarray(sigs).tobytes()
    if kind == "domain":
        ok, bm, comb, re_ = eng.g1pubs_verify_with_domain_batch_rlc_grouped_locate(table, DOMAIN, msg_idx, p, s, inf, scalars, block)
    else:
        fn = eng.g2pubs_verify_batch_rlc_grouped_locate if kind == "g2pubs" else eng.g1pubs_verify_batch_rlc_grouped_locate
        ok, bm, comb, re_ = fn(table, msg_idx, p, s, inf, scalars, block)
    assert np.array_equal(bm, np.packbits(np.asarray(ok, np.uint8), bitorder="little")[:len(bm)])
    return [bool(x) for x in ok], comb, re_


def gl_jac(eng, kind, table, msg_idx, pj, sj, scalars=None, block=BLOCK):
    if kind == "domain":
        ok, _, comb, re_ = eng.g1pubs_verify_with_domain_batch_rlc_grouped_locate_jac(table, DOMAIN, msg_idx, pj, sj, scalars, block)
    else:
        fn = eng.g2pubs_verify_batch_rlc_grouped_locate_jac if kind == "g2pubs" else eng.g1pubs_verify_batch_rlc_grouped_locate_jac
        ok, _, comb, re_ = fn(table, msg_idx, pj, sj, scalars, block)
    return [bool(x) for x in ok], comb, re_


def _cells(msg_idx, block):
    """the cells as lists of tuple positions"""
    perm, cells = cells_mirror(msg_idx, block)
    return [[perm[k] for k in range(lo, hi)] for lo, hi, _ in cells]


def _sizes_of_cells_with(msg_idx, block, bad):
    return sum(len(c) for c in _cells(msg_idx, block) if any(i in bad for i in c))


def _cell_of(msg_idx, block, i):
    return next(c for c in _cells(msg_idx, block) if i in c)


def oracle_cell(kind, msg, pks, sigs, r, members):
    """the equation of one cell -- the tuples `members`, all of message msg -- composed from the oracle's primitives"""
    k32 = {i: int(r[i]).to_bytes(32, "big") for i in members}
    m = len(members)
    if kind == "g2pubs":
        S = RC.g1_sum(b"".join(RC.g1_mul(bytes(sigs[i]), k32[i]) for i in members), m)
        K = RC.g2_sum(b"".join(RC.g2_mul(bytes(pks[i]), k32[i]) for i in members), m)
        lhs = _fe(RC.miller_loop(S, RC.g2_generator(), 1))
        rhs = _fe(RC.miller_loop(RC.hash_g1(msg), K, 1))
    else:
        S = RC.g2_sum(b"".join(RC.g2_mul(bytes(sigs[i]), k32[i]) for i in members), m)
        K = RC.g1_sum(b"".join(RC.g1_mul(bytes(pks[i]), k32[i]) for i in members), m)
        lhs = _fe(RC.miller_loop(RC.g1_generator(), S, 1))
        rhs = _fe(RC.miller_loop(K, RC.hash_g2(msg) if kind == "g1pubs" else RC.hash_g2_with_domain(msg, DOMAIN), 1))
    return bool(np.array_equal(lhs, rhs))


def test_the_base_shape_is_what_the_docstring_says():
    for n in (70, 71):
        idx = _interleaved(SIZES[n])
        assert len(idx) == n and sorted(set(idx)) == [0, 1, 3, 4, 5] and cells_mirror(idx, BLOCK)[0] != list(range(n))
        assert [len(c) for c in _cells(idx, BLOCK)] == [1, 2, 4, 4, 1] + [4] * 6 + [1] + [4] * 8 + [n - 69]


# ---- 1. all valid ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_all_valid_affine_and_in_memory(eng, kind):
    for n in (N, N + 1):
        table, idx, pks, sigs = _batch(eng, kind, n)
        ok, comb, re_ = gl(eng, kind, table, idx, pks, sigs)
        assert all(ok) and len(ok) == n and comb == 1 and re_ == 0, (kind, n)
        pj, sj = _jac_forms(kind, pks, sigs, n)
        ok, comb, re_ = gl_jac(eng, kind, table, idx, b"".join(pj), b"".join(sj))
        assert all(ok) and len(ok) == n and comb == 1 and re_ == 0, (kind, n, "in-memory")
    ok, comb, re_ = gl(eng, kind, table, idx[:1], pks[:1], sigs[:1], block=0)     # one tuple, the automatic block
    assert ok == [True] and comb == 1 and re_ == 0


# ---- 2. corruptions ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_corruptions_recheck_their_cells_only(eng, kind):
    table, idx, pks, sigs = _batch(eng, kind)
    for block in (4, 1, 2, 40, 1024):
        cells = _cells(idx, block)
        wide = [c for c in cells if len(c) >= 2]
        two = set(wide[-1][:2]) if wide else set(cells[-1] + cells[-2])          # two tuples of one cell (block = 1: of one group)
        for bad in (two, {c[0] for c in cells}, {17}):
            ix = list(idx); p = pks.copy(); s = sigs.copy()
            for j, i in enumerate(sorted(bad)):
                if j % 3 == 0:
                    ix[i] = (ix[i] + 1) % D                                       # wrong message-table index (entry 2 gets its first tuple)
                elif j % 3 == 1:
                    p[i] = pks[(i + 1) % N]                                       # wrong key
                else:
                    s[i] = np.frombuffer(_rand_sig_point(kind, i), np.uint8)      # tampered signature
            ok, comb, re_ = gl(eng, kind, table, ix, p, s, block=block)
            assert comb == 0, (kind, block, sorted(bad))
            assert ok == vb(eng, kind, expand(table, ix), p, s) == [i not in bad for i in range(N)], (kind, block, sorted(bad))
            assert re_ == _sizes_of_cells_with(ix, block, bad), (kind, block, sorted(bad), re_)
            if block == 4 and bad == two:
                for i in sorted(bad):
                    assert oracle_verify(kind, table[ix[i]], p[i], s[i]) is False and oracle_verify(kind, table[idx[i]], pks[i], sigs[i]) is True, (kind, i)


# ---- 3. the cell arithmetic, pinned by caller scalars -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_cell_arithmetic_pinned_by_caller_scalars(eng, kind):
    n = N + 1
    table, idx, pks, sigs = _batch(eng, kind, n)
    cells = _cells(idx, BLOCK)
    big = [c for c in cells if idx[c[0]] == 5]                                    # the group of 34: 8 cells of 4 and one of 2
    assert [len(c) for c in big] == [4] * 8 + [2]
    rnd = random.Random(41)
    r = [rnd.randrange(1, 1 << 64) for _ in range(n)]
    r[big[0][0]], r[big[0][1]], r[big[0][2]] = 1, 1 << 63, (1 << 64) - 1
    a, c, w = big[2][1], big[8][0], next(cl for cl in cells if idx[cl[0]] == 3)[0]   # two cells of one group (the ragged one among them), and a cell of 4 elsewhere
    r[c] = r[a]
    Dp = _rand_sig_point(kind, 7)
    s = sigs.copy()
    s[a] = np.frombuffer(_sig_add(kind, sigs[a], Dp), np.uint8)
    s[c] = np.frombuffer(_sig_add(kind, sigs[c], _neg(kind, Dp)), np.uint8)
    p = pks.copy(); p[w] = pks[(w + 1) % n]
    want_cells = [oracle_cell(kind, table[idx[cl[0]]], p, s, r, cl) for cl in cells]
    assert want_cells == [not any(i in (a, c, w) for i in cl) for cl in cells]
    ok, comb, re_ = gl(eng, kind, table, idx, p, s, scalars=r)
    assert comb == 0 and re_ == 4 + 2 + 4, (kind, comb, re_)
    assert ok == [i not in (a, c, w) for i in range(n)] == vb(eng, kind, expand(table, idx), p, s)
    # without the wrong key the total holds under these scalars (r_a D - r_c D = 0), though two of its cells would not: nothing is rechecked
    ok, comb, re_ = gl(eng, kind, table, idx, pks, s, scalars=r)
    assert comb == 1 and all(ok) and re_ == 0
    ok, comb, re_ = gl(eng, kind, table, idx, pks, s)                             # drawn scalars: caught, in two cells
    assert comb == 0 and re_ == 6 and ok == [i not in (a, c) for i in range(n)]


@pytest.mark.parametrize("kind", ("g2pubs", "g1pubs"))
def test_same_pair_inside_one_cell(eng, kind):
    table, idx, pks, sigs = _batch(eng, kind)
    cells = _cells(idx, BLOCK)
    cell = [cl for cl in cells if idx[cl[0]] == 4][3]                             # a full cell of the group of 25
    a, c = cell[0], cell[3]
    r = [3 + 2 * i for i in range(N)]
    r[c] = r[a]
    Dp = _rand_sig_point(kind, 9)
    s = sigs.copy()
    s[a] = np.frombuffer(_sig_add(kind, sigs[a], Dp), np.uint8)
    s[c] = np.frombuffer(_sig_add(kind, sigs[c], _neg(kind, Dp)), np.uint8)
    assert oracle_cell(kind, table[4], pks, s, r, cell)
    ok, comb, re_ = gl(eng, kind, table, idx, pks, s, scalars=r)                  # the documented caveat of caller scalars
    assert comb == 1 and all(ok) and re_ == 0
    w = next(cl for cl in cells if idx[cl[0]] == 5)[2]                            # the total fails elsewhere: the cell still holds, as its equation does
    p = pks.copy(); p[w] = pks[(w + 1) % N]
    ok, comb, re_ = gl(eng, kind, table, idx, p, s, scalars=r)
    assert comb == 0 and re_ == 4 and ok == [i != w for i in range(N)]
    ok, comb, re_ = gl(eng, kind, table, idx, pks, s)                             # drawn scalars catch it
    assert comb == 0 and re_ == 4 and ok == [i not in (a, c) for i in range(N)]


# ---- 4. infinity --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_infinity_fails_its_cell_only(eng, kind):
    table, idx, pks, sigs = _batch(eng, kind)
    msgs = expand(table, idx)
    size = lambda i: len(_cell_of(idx, BLOCK, i))                                 # noqa: E731
    for i, flag in ((12, 1), (69, 2), (idx.index(0), 1)):                         # a flagged key, a flagged signature, the single-tuple group
        inf = np.zeros(N, np.uint8); inf[i] = flag
        ok, comb, re_ = gl(eng, kind, table, idx, pks, sigs, inf=inf)
        assert comb == 0 and ok == [j != i for j in range(N)] == vb(eng, kind, msgs, pks, sigs, inf), (kind, i)
        assert re_ == size(i), (kind, i, re_)
    p = pks.copy(); p[33] = 0                                                     # the all-zero record
    ok, comb, re_ = gl(eng, kind, table, idx, p, sigs)
    assert comb == 0 and re_ == size(33) and ok == [j != 33 for j in range(N)]
    s = sigs.copy(); s[0] = 0
    ok, comb, re_ = gl(eng, kind, table, idx, pks, s, block=2)
    assert comb == 0 and re_ == len(_cell_of(idx, 2, 0)) and ok == [j != 0 for j in range(N)]
    pj, sj = _jac_forms(kind, pks, sigs, 3)
    sj[41] = g1_to_jac(None) if kind == "g2pubs" else g2_to_jac(None)             # z = 0
    ok, comb, re_ = gl_jac(eng, kind, table, idx, b"".join(pj), b"".join(sj))
    assert comb == 0 and re_ == size(41) and ok == [j != 41 for j in range(N)]


def _neg_key(kind, pt):
    return _neg("g1pubs" if kind == "g2pubs" else "g2pubs", pt)                   # (keys live in the other group than signatures)


@pytest.mark.parametrize("kind", ("g2pubs", "g1pubs"))
def test_cell_sums_at_infinity(eng, kind):
    table, idx, pks, sigs = _batch(eng, kind)
    a, b = [cl for cl in _cells(idx, 2) if idx[cl[0]] == 4][5]                    # a cell of two tuples at block = 2
    r = [5 + i for i in range(N)]
    r[b] = r[a]
    s = sigs.copy(); s[b] = np.frombuffer(_neg(kind, bytes(sigs[a])), np.uint8)   # S_c = r_a sig_a + r_b (-sig_a) = 0
    ok, comb, re_ = gl(eng, kind, table, idx, pks, s, scalars=r, block=2)
    assert comb == 0 and re_ == 2 and ok == [j != b for j in range(N)] == vb(eng, kind, expand(table, idx), pks, s)
    p = pks.copy(); p[b] = np.frombuffer(_neg_key(kind, bytes(pks[a])), np.uint8)  # K_c = r_a pk_a + r_b (-pk_a) = 0
    ok, comb, re_ = gl(eng, kind, table, idx, p, sigs, scalars=r, block=2)
    assert comb == 0 and re_ == 2 and ok == [j != b for j in range(N)] == vb(eng, kind, expand(table, idx), p, sigs)


# ---- 5. a cell larger than 64 tuples: the fold passes of the segmented sums ---------------------------------------------------------------
@pytest.mark.parametrize("kind", ("g2pubs", "g1pubs"))
def test_cells_beyond_one_wave_of_partials(eng, kind):
    n = 500
    table, idx, pks, sigs = _batch(eng, kind, n, sizes=(450, 49, 1))
    cells = _cells(idx, 200)
    assert [len(c) for c in cells] == [200, 200, 50, 49, 1]
    bad = {cells[1][77], cells[4][0]}
    s = sigs.copy()
    for i in bad:
        s[i] = np.frombuffer(_rand_sig_point(kind, i), np.uint8)
    ok, comb, re_ = gl(eng, kind, table, idx, pks, s, block=200)
    assert comb == 0 and re_ == 201 and ok == [i not in bad for i in range(n)], (kind, comb, re_)
    ok, comb, re_ = gl(eng, kind, table, idx, pks, sigs, block=200)
    assert comb == 1 and re_ == 0 and all(ok)


# ---- 6. layouts ---------------------------------------------------------------------------------------------------------------------
def test_layouts_give_identical_results(eng):
    from bls_amd import _native
    lib = _native.load()
    n = N + 1
    settings = {"k_lat:miller1raw": lambda: None,
                "k_miller1h_row": lambda: eng.set_row_threshold(1, 1 << 20),
                "k_miller1h_quad": lambda: (eng.set_row_threshold(0, 0), eng.set_latency_threshold(0)),
                "k_miller1h_pair": lambda: (eng.set_row_threshold(0, 0), eng.set_latency_threshold(0), eng.set_quad_threshold(0))}
    fe_seen = set()
    for kind in ("g2pubs", "g1pubs"):
        table, idx, pks, sigs = _batch(eng, kind, n)
        cells = _cells(idx, BLOCK)
        bad = {cells[3][1], cells[-1][1]}                                         # cell 3 (four tuples; its neighbour, cell 4, has one and stays valid) and the ragged last one
        p = pks.copy()
        for i in bad:
            p[i] = pks[(i + 1) % n]
        for block in (BLOCK, 1):
            want_re = _sizes_of_cells_with(idx, block, bad)
            for name, apply in settings.items():
                try:
                    apply()
                    lib.blsmi_set_profiling(1)
                    _profile(lib)
                    ok, comb, re_ = gl(eng, kind, table, idx, p, sigs, block=block)
                    prof = _profile(lib)
                    okv, combv, rev = gl(eng, kind, table, idx, pks, sigs, block=block)
                finally:
                    lib.blsmi_set_profiling(0)
                    eng.set_latency_threshold(8192); eng.set_quad_threshold(16384); eng.set_row_threshold(*eng.ROW_DEFAULT)
                for want in (name, "k_locate_cell_fail", "k_locate_sig_pairs", "k_fq12_mul_pairs_row", "k_fq12_is_one_m384", "k_gather_records16", "k_scatter_bytes",
                             "k_g2_segsum_chunk_u64", "k_g1_segsum_chunk_u64"):
                    assert want in prof, (kind, block, name, want, prof)
                assert prof.count(name) >= 2, (kind, block, name, prof)           # the cells' tuple side and their signature side
                # one value per cell in every layout: cells 3 and 4 merged into one value would recheck 4 + 1 tuples for the bad tuple of cell 3
                assert comb == 0 and re_ == want_re and ok == [i not in bad for i in range(n)], (kind, block, name, re_)
                assert combv == 1 and rev == 0 and all(okv), (kind, block, name)
                fe_seen |= set(prof) & {"k_lat:finalexp1", "k_final_exp_row", "k_final_exp_quad", "k_final_exp_pair"}
    assert {"k_lat:finalexp1", "k_final_exp_row"} <= fe_seen, fe_seen


# ---- 7. segsum_chunk ------------------------------------------------------------------------------------------------------------------
def test_segsum_chunk_option(eng):
    kind = "g1pubs"
    table, idx, pks, sigs = _batch(eng, kind)
    bad = {9, 64}
    p = pks.copy()
    for i in bad:
        p[i] = pks[i + 1]
    got = []
    try:
        for k in (0, 2, 1024):
            eng.set_option("segsum_chunk", k)
            got.append(gl(eng, kind, table, idx, p, sigs, block=40))
    finally:
        eng.set_option("segsum_chunk", 0)
    assert got[0] == got[1] == got[2]
    assert got[0] == ([i not in bad for i in range(N)], 0, _sizes_of_cells_with(idx, 40, bad))


# ---- 8. the call that holds -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("g2pubs", "g1pubs"))
def test_the_call_that_holds_runs_no_cell_check(eng, kind):
    from bls_amd import _native
    lib = _native.load()
    table, idx, pks, sigs = _batch(eng, kind, N + 1)
    try:
        lib.blsmi_set_profiling(1)
        _profile(lib)
        ok, comb, re_ = gl(eng, kind, table, idx, pks, sigs)
        prof = _profile(lib)
    finally:
        lib.blsmi_set_profiling(0)
    assert comb == 1 and all(ok) and re_ == 0
    assert not [x for x in prof if x.startswith("k_locate_")], prof
    assert not [x for x in prof if "final_exp" in x or "finalexp" in x], prof     # (the tail program is the one final exponentiation)
    assert not [x for x in prof if "gather" in x or "scatter" in x], prof
    assert prof[-1] == "k_lat:aggtail2" and "k_fq12_mul_pairs_row" not in prof
    assert "k_g1_segsum_chunk_u64" in prof and "k_g2_segsum_chunk_u64" in prof and "k_lat:miller1raw" in prof, prof   # both sides are summed per cell
    assert not [x for x in prof if "msm" in x or x in ("k_g1_mul_u64", "k_g2_mul_u64")], prof


# ---- 9. concurrency -------------------------------------------------------------------------------------------------------------------
def test_concurrent_mixed_calls(eng):
    n_pool, d = 320, 7
    pool = {k: _gbatch(eng, k, n_pool, d, seed=55) for k in ("g2pubs", "g1pubs")}
    rlc_min = _default_rlc_min()
    errors = []

    def worker(tid):
        rnd = random.Random(100 + tid)
        try:
            for it in range(4):
                k = ("g2pubs", "g1pubs")[(tid + it) % 2]
                table, idx, pks, sigs = pool[k]
                n = rnd.randrange(280, 320)
                ix = list(idx[:n]); p = pks[:n].copy(); s = sigs[:n]
                bad = set(rnd.sample(range(n), rnd.randrange(1, 4))) if rnd.random() < 0.6 else set()
                for i in bad:
                    p[i] = pks[(i + 1) % n]
                want = [i not in bad for i in range(n)]
                which = (tid + it) % 4
                if which == 0:
                    block = rnd.choice((0, 1, 5, 64))
                    ok, comb, re_ = gl(eng, k, table, ix, p, s, block=block)
                    if comb != (0 if bad else 1) or re_ != _sizes_of_cells_with(ix, block, bad):
                        errors.append((tid, it, "grouped_locate", comb, re_, sorted(bad)))
                elif which == 1:
                    ok, comb = grouped(eng, k, table, ix, p, s)
                elif which == 2:
                    ok, comb, re_ = locate(eng, k, expand(table, ix), p, s, block=8)
                else:
                    ok = vb(eng, k, expand(table, ix), p, s)
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
