"""-m gpu: the group law's rare branches, bit for bit against the C oracle (whose own special cases tests/test_group_edges_cpu.py checks
against the Python twin).  Operands come from tests/group_edges.py: the same point and opposite points under many Z, infinite operands,
G2 points whose x agree in one coefficient only, crafted records whose h or rr0 is zero in one coefficient only.

Which code each test reaches:
  debug ops G?_ADD / G?_DOUBLE            jac_add / jac_double, one point per lane
  g2_sum_segmented                        the LANE-PAIR instance: k_g2_segsum_chunk_pair (mixed addition; segsum_chunk 1024 puts a whole segment
                                          on one lane pair) and k_g2_segsum_fold_pair (general addition; segsum_chunk 1 makes every point a partial)
  g1_sum_segmented, g?_sum_segmented_jac  the one-lane chunk kernels, k_g1_segsum_fold, k_g?_segsum_final (a shuffle tree across one wave)
  g?_sum_segmented_u64                    k_g?_segsum_chunk_u64, then the same folds
  g?_sum, g?_sum_jac, sum_dev             up to 2 x lat_max points (16 384 by default) the level programs of k_lat.hip; with the latency threshold at 0
                                          k_g?_sum0 (k_g?_sum0_jac), one k_g?_sum launch per further level, k_g?_sum_final -- see test_tree_sums
  g?_mul_batch / g?_msm, any-point flag   k_g1_mul, and for G2 the lane-pair k_g2_mul_pair; the MSM adds the multiples through the tree sum
  the any-point MSM from BLSMI_MSM_BUCKET_MIN points on: k_g2_msm_bucket_pair (a child process: the variable is read at start-up)

Every count handed to a kernel is odd and above 64 (a ragged last workgroup, more than one wave) wherever the entry point takes a count of
records; the tree sums take the n that their docstring lists."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":                                                   # the child process of test_bucket_kernel_...: python tests/<this file>
    sys.path.insert(0, ROOT)

import group_edges as G
from gpu_common import P, RC

pytestmark = pytest.mark.gpu

GROUPS = (1, 2)
NAME = {1: "g1", 2: "g2"}
PB = G.PB
ADD = {1: RC.g1_add, 2: RC.g2_add}
DBL = {1: RC.g1_double, 2: RC.g2_double}
TO_AFF = {1: RC.g1_jac_to_affine_bytes, 2: RC.g2_jac_to_affine_bytes}
OSUM = {1: RC.g1_sum, 2: RC.g2_sum}
OMUL = {1: RC.g1_mul, 2: RC.g2_mul}
LAT_DEFAULT = 8192
CHUNKS = (1, 0, 1024)


@pytest.fixture(scope="module")
def eng():
    from bls_amd import engine
    engine.init(0)
    yield engine
    engine.set_latency_threshold(LAT_DEFAULT); engine.set_option("segsum_chunk", 0)


def _dev(b):
    import torch
    a = np.ascontiguousarray(b) if isinstance(b, np.ndarray) else np.frombuffer(bytes(b), dtype=np.uint8)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(torch.device("cuda", 0))


def _zeros(nbytes):
    import torch
    return torch.zeros(nbytes, dtype=torch.uint8, device=torch.device("cuda", 0))


def _neg_wire(group, w):
    return G.wire(group, G.neg(group, G.unwire(group, w)))


def _osum(group, pts, flags=None):
    """the oracle's sum of wire records (None entries are left out) -> wire bytes or None"""
    if flags is not None:
        pts = [p for p, f in zip(pts, flags) if not f]
    pts = [p for p in pts if p is not None]
    return OSUM[group](b"".join(pts), len(pts)) if pts else None


_MUL = {}


def _omul(group, w, k):
    """the oracle's multiple k * point, cached (every call of RC.g?_mul of this file goes through here)"""
    if k == 1:
        return w                                                             # (an affine point is its own multiple by 1)
    key = (group, w, k)
    if key not in _MUL:
        _MUL[key] = OMUL[group](w, k.to_bytes(32, "big"))
    return _MUL[key]


# ---- 1. the debug ops: jac_add and jac_double, one point per lane ----------------------------------------------------------------------
def _check_points(group, got, want, labels, what):
    z = slice(2 * G.WIDTH[group] // 3, G.WIDTH[group])
    bad = []
    for i in range(len(want)):
        w = TO_AFF[group](want[i])
        if TO_AFF[group](got[i]) != w or (w is None and got[i][z].any()):   # the same point; and Z exactly zero where the oracle's sum is infinite
            bad.append((i, labels[i]))
    assert not bad, (NAME[group], what, len(bad), bad[:8])


@pytest.mark.parametrize("group", GROUPS)
def test_additions_on_the_whole_corpus_in_both_orders(eng, group):
    corpus = G.corpus(group)
    labels = [c.label for c in corpus]
    a, b = G.records(group, [c.p for c in corpus]), G.records(group, [c.q for c in corpus])
    assert len(a) % 2 == 1 and len(a) > 64
    for x, y, what in ((a, b, "p + q"), (b, a, "q + p")):
        out, _ = eng.debug_op("G%d_ADD" % group, x, y)
        _check_points(group, out, [ADD[group](u, v) for u, v in zip(x, y)], labels, what)


@pytest.mark.parametrize("group", GROUPS)
def test_doublings_of_every_first_operand_and_of_infinity(eng, group):
    labels, ops = G.doubling_operands(group)
    a = G.records(group, ops)
    out, _ = eng.debug_op("G%d_DOUBLE" % group, a)
    _check_points(group, out, [DBL[group](u) for u in a], labels, "2 p")


# ---- 2. segmented sums -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _segment_wants(group):
    case = G.sum_case(group)
    return [G.oracle_segment_sum(group, case, s) for s in case.segs]


def _check_segments(group, out, oinf, want, labels, what):
    pb = PB[group]
    bad = [(j, labels[j]) for j, w in enumerate(want) if oinf[j] != (w is None) or out[pb * j:pb * (j + 1)] != (bytes(pb) if w is None else w)]
    assert not bad, (NAME[group], what, len(bad), bad[:8])


@pytest.mark.parametrize("group", GROUPS)
def test_segmented_sums_meet_every_exceptional_pair(eng, group):
    """One segment [P, Q] per corpus pair, the three-element and the long segments of group_edges.sum_case, through the affine form (G2: the
    lane-pair kernels -- the class-d pairs are the only route by which a partially zero h reaches them), the in-memory form (the same points
    under differing Z) and the resident form, at segsum_chunk 1 (every pair meets in a fold's or the final kernel's general addition), 0 and
    1024 (in the chunk kernel's mixed addition): the same bytes at all three, the oracle's."""
    import torch
    case, want = G.sum_case(group), _segment_wants(group)
    npk, m, pb = len(case.table), len(case.segs), PB[group]
    assert npk % 2 == 1 and m % 2 == 1 and m > 64
    idx = np.array([i for s in case.segs for i in s], dtype=np.uint32)
    off = eng.seg_offsets([len(s) for s in case.segs])
    table, jtab = b"".join(case.table), b"".join(case.jtab)
    flags = case.inf.copy()
    flags[[i for i, w in enumerate(case.table) if w == bytes(pb)]] = 0      # the all-zero record says infinity by itself
    assert flags.any() and (flags != case.inf).any()
    aff, jac = (eng.g1_sum_segmented, eng.g1_sum_segmented_jac) if group == 1 else (eng.g2_sum_segmented, eng.g2_sum_segmented_jac)
    d_p, d_f, d_x, d_o = _dev(table), _dev(flags), _dev(idx), _dev(off)
    results = []
    try:
        for K in CHUNKS:
            eng.set_option("segsum_chunk", K)
            out, oinf = aff(table, npk, idx, off, flags)
            _check_segments(group, out, oinf, want, case.labels, ("affine", K))
            jo, ji = jac(jtab, npk, idx, off)
            _check_segments(group, jo, ji, want, case.labels, ("in-memory", K))
            d_out, d_inf = _zeros(pb * m), _zeros(m)
            eng.sum_segmented_dev(NAME[group], d_p.data_ptr(), d_f.data_ptr(), npk, d_x.data_ptr(), d_o.data_ptr(), m, d_out.data_ptr(), d_inf.data_ptr())
            torch.cuda.synchronize()
            _check_segments(group, d_out.cpu().numpy().tobytes(), d_inf.cpu().numpy(), want, case.labels, ("resident", K))
            results.append(out)
    finally:
        eng.set_option("segsum_chunk", 0)
    assert results[0] == results[1] == results[2]


# ---- 3. weighted segmented sums --------------------------------------------------------------------------------------------------------
U64 = (1 << 64) - 1


@functools.lru_cache(maxsize=None)
def _weighted_case(group):
    """(table, weights, segments, wants): every (weight, point) of a segment is a table entry of its own (the weight is addressed by the
    point's index); subgroup points only -- the weighted form multiplies"""
    xs = P.XORShift(9400 + group)
    table, weights, segs, want, labels = [], [], [], [], []

    def add(label, *terms):
        seg = []
        for w, p in terms:
            seg.append(len(table)); table.append(p); weights.append(w)
        segs.append(seg); labels.append(label)
        want.append(_osum(group, [_omul(group, p, w) if w else None for w, p in terms]))

    pts = [G.wire(group, a) for a in G.subgroup_points(group)]
    for i in range(3):
        p, q, r = pts[i], pts[i + 3], pts[(i + 1) % 3]
        n = _neg_wire(group, p)
        rw = (P.rand_int(xs, U64 - 1) + 1, P.rand_int(xs, U64 - 1) + 1)
        for w in (1, 2, 1 << 63, U64) + rw:
            add("w P, w P", (w, p), (w, p))
            add("w P, w -P", (w, p), (w, n))
        for w in (1, 1 << 63, U64):                                          # the same group element by two routes (different Z), on either side
            wp = _omul(group, p, w)
            add("w P, 1 (wP)", (w, p), (1, wp))
            add("1 (wP), w P", (1, wp), (w, p))
            add("w P, 1 -(wP)", (w, p), (1, _neg_wire(group, wp)))
            add("1 -(wP), w P, R", (1, _neg_wire(group, wp)), (w, p), (rw[0], r))
        add("2 P, 1 (2P)", (2, p), (1, _omul(group, p, 2)))
        add("3 P, 1 -(3P)", (3, p), (1, _neg_wire(group, _omul(group, p, 3))))
        add("0 P, w Q", (0, p), (rw[0], q))
        add("w P, 0 Q", (rw[0], p), (0, q))
        add("all weights 0", (0, p), (0, q), (0, r))
        add("w P, w P, w -P, w -P", (rw[1], p), (rw[1], p), (rw[1], n), (rw[1], n))
    if len(segs) % 2 == 0:
        add("w P", (rw[0], pts[0]))
    assert len(segs) % 2 == 1 and len(segs) > 64
    return tuple(table), tuple(weights), tuple(tuple(s) for s in segs), tuple(want), tuple(labels)


@pytest.mark.parametrize("group", GROUPS)
def test_weighted_segmented_sums_meet_equal_and_opposite_products(eng, group):
    table, weights, segs, want, labels = _weighted_case(group)
    fn = eng.g1_sum_segmented_u64 if group == 1 else eng.g2_sum_segmented_u64
    idx = np.array([i for s in segs for i in s], dtype=np.uint32)
    off = eng.seg_offsets([len(s) for s in segs])
    assert sum(1 for w in want if w is None) >= 20
    results = []
    try:
        for K in CHUNKS:
            eng.set_option("segsum_chunk", K)
            out, oinf = fn(b"".join(table), len(table), list(weights), idx, off)
            _check_segments(group, out, oinf, want, labels, ("weighted", K))
            results.append(out)
    finally:
        eng.set_option("segsum_chunk", 0)
    assert results[0] == results[1] == results[2]


# ---- 4. tree sums ----------------------------------------------------------------------------------------------------------------------
TREE_N = (2, 3, 4, 64, 65, 128, 129, 4097)


def tree_levels(n):
    """The reduction of sum_dev (blsmi.hip), which k_g?_sum0 / k_g?_sum and the level programs share: level 0 adds input t + half to input t
    (half = ceil(n / 2)), every further level does the same to the partial sums.  -> per level the list of (indices summed in the left
    operand, indices summed in the right operand), one entry per addition."""
    cur = [[i] for i in range(n)]
    levels = []
    while len(cur) > 1:
        half = (len(cur) + 1) // 2
        levels.append([(cur[t], cur[t + half]) for t in range(half) if t + half < len(cur)])
        cur = [cur[t] + (cur[t + half] if t + half < len(cur) else []) for t in range(half)]
    return levels


@functools.lru_cache(maxsize=None)
def _distinct_points(group):
    """max(TREE_N) distinct subgroup points as wire records and as in-memory records under differing Z: P_0 + i G by oracle additions"""
    xs = P.XORShift(9500 + group)
    gen = RC.g1_generator() if group == 1 else RC.g2_generator()
    pts = [G.wire(group, G.subgroup_points(group)[0])]
    while len(pts) < max(TREE_N):
        pts.append(OSUM[group](pts[-1] + gen, 2))
    zs = [G.rand_z(group, xs) for _ in range(61)]
    jac = [G.record(group, G.scale(group, G.unwire(group, w), zs[i % 61])).tobytes() for i, w in enumerate(pts)]
    return pts, jac


def _tree_arrays(group, n):
    """for every level of the reduction three arrays: in one addition of that level the operands are equal sums, opposite sums, or one of
    them an all-infinite half -> (label, points, infinity flags)"""
    base = _distinct_points(group)[0][:n]
    out = []
    for L, adds in enumerate(tree_levels(n)):
        left, right = adds[0] if L % 2 == 0 else adds[-1]                    # the first addition of the level, or its last (next to the ragged end)
        rest = [base[i] for i in right[:-1]]
        t = _osum(group, [base[i] for i in left])
        for label, target in (("equal", t), ("opposite", _neg_wire(group, t))):
            pts = list(base)
            pts[right[-1]] = _osum(group, [target] + [_neg_wire(group, p) for p in rest])
            out.append(("%s sums at level %d" % (label, L), pts, np.zeros(n, dtype=np.uint8)))
        flags = np.zeros(n, dtype=np.uint8)
        flags[left if L % 4 >= 2 else right] = 1
        out.append(("an all-infinite half at level %d" % L, list(base), flags))
    return out


@pytest.mark.parametrize("n", TREE_N)
@pytest.mark.parametrize("group", GROUPS)
def test_tree_sums_meet_an_exceptional_pair_at_every_level(eng, group, n):
    """g?_sum, g?_sum_jac and sum_dev over arrays in which an addition of equal sums, of opposite sums or with an all-infinite operand first
    happens at level 0, 1, ... of the reduction (tree_levels), infinity given by the in_inf flags, by the all-zero record and by Z = 0.
    Each array runs twice.  With the default latency threshold every n here is summed by the level programs of k_lat.hip (sum0, sum1 per
    further level, sumfin: up to 16 384 points).  With the threshold at 0 the kernels run: n = 2 reaches k_g?_sum0 (k_g?_sum0_jac for the
    in-memory form) and k_g?_sum_final only; n = 3 and 4 add one launch of k_g?_sum; 64 -> 5 launches, 65 and 128 -> 6, 129 -> 7, 4097 -> 12
    launches of k_g?_sum between k_g?_sum0 and k_g?_sum_final, the odd n with a ragged level (an operand without a partner) on the way."""
    assert len(tree_levels(n)) == (n - 1).bit_length() and sum(len(a) for a in tree_levels(n)) == n - 1
    pb = PB[group]
    base, base_jac = (a[:n] for a in _distinct_points(group))
    xs = P.XORShift(9700 + group)
    fsum, fjac = (eng.g1_sum, eng.g1_sum_jac) if group == 1 else (eng.g2_sum, eng.g2_sum_jac)
    zero_jac = G.record(group, G.infinities(group, xs)[0]).tobytes()
    d_out = _zeros(pb)
    try:
        for label, pts, flags in _tree_arrays(group, n):
            want = _osum(group, pts, flags)
            zeroed = [bytes(pb) if f else p for p, f in zip(pts, flags)]
            jac = [zero_jac if f else (base_jac[i] if p is base[i] else G.record(group, G.scale(group, G.unwire(group, p), G.rand_z(group, xs))).tobytes())
                   for i, (p, f) in enumerate(zip(pts, flags))]
            d_p, d_z, d_f = _dev(b"".join(pts)), _dev(b"".join(zeroed)), _dev(flags)
            for lat in (LAT_DEFAULT, 0):
                eng.set_latency_threshold(lat)
                what = (NAME[group], n, label, lat)
                assert fsum(b"".join(pts), n, flags if flags.any() else None) == want, what
                if flags.any():
                    assert fsum(b"".join(zeroed), n) == want, what + ("zero records",)
                jo, ji = fjac(b"".join(jac), n)
                assert ji == (want is None) and TO_AFF[group](np.frombuffer(jo, dtype=np.uint64)) == want, what + ("in-memory",)
                for d_pts, d_flags in ((d_p, d_f), (d_z, None)) if flags.any() else ((d_p, None),):
                    inf = eng.sum_dev(NAME[group], d_pts.data_ptr(), d_flags.data_ptr() if d_flags is not None else 0, n, d_out.data_ptr())
                    assert inf == (want is None) and (inf or d_out.cpu().numpy().tobytes() == want), what + ("resident",)
    finally:
        eng.set_latency_threshold(LAT_DEFAULT)


# ---- 5. scalar multiplication of any curve point -----------------------------------------------------------------------------------------
R = P.R_ORDER


@functools.lru_cache(maxsize=None)
def _any_point_case(group):
    """(points, scalars): G2 -- two class-d pairs (x agree in c0 / in c1) and points with x.c0 = 0 and x.c1 = 0, all outside the subgroup;
    G1 -- the points with x = 0, two more outside the subgroup and two inside"""
    xs = P.XORShift(9800 + group)
    if group == 2:
        pools = G.partial_pools()
        pts = list(pools["c0"][0][:2]) + list(pools["c1"][0][:2]) + list(pools["c0"][1][:2]) + list(pools["c1"][1][:2])
    else:
        pts = list(G.x_zero_points(1)) + list(G.outside_points(1)[:2]) + list(G.subgroup_points(1)[:2])
    scalars = [0, 1, 2, 3, R - 1, R, R + 1, 1 << 255, (1 << 256) - 1] + [P.rand_int(xs, 1 << 256) for _ in range(3)]
    return [G.wire(group, a) for a in pts], scalars


@pytest.mark.parametrize("group", GROUPS)
def test_any_point_multiples_of_partial_zero_and_x_zero_points(eng, group):
    pts, scalars = _any_point_case(group)
    pb = PB[group]
    items = [(p, k) for p in pts for k in scalars] + [(pts[0], 5)]
    n = len(items)
    assert n % 2 == 1 and n > 64
    fn = eng.g1_mul_batch if group == 1 else eng.g2_mul_batch
    out, inf = fn(b"".join(p for p, _ in items), b"".join(k.to_bytes(32, "big") for _, k in items), n, any_point=True)
    bad = []
    for i, (p, k) in enumerate(items):
        w = _omul(group, p, k)
        if bool(inf[i]) != (w is None) or out[i].tobytes() != (bytes(pb) if w is None else w):
            bad.append((i, i // len(scalars), hex(k)))
    assert not bad, (NAME[group], len(bad), bad[:8])


@pytest.mark.parametrize("group", GROUPS)
def test_any_point_msm_below_the_bucket_threshold_adds_a_partial_zero_pair(eng, group):
    """equal scalars on two points whose x agree in one coefficient (G1: on the two points with x = 0): their multiples by 1 meet in the final
    sum with a partially zero h; n = 2, and n = 67 with the pair at t and t + half of the tree's first level"""
    pts, scalars = _any_point_case(group)
    fn = eng.g1_msm if group == 1 else eng.g2_msm
    cases = []
    for a, b in ((0, 1), (2, 3)):
        for k in (1, 3, R - 1, scalars[-1]):
            cases.append(([pts[a], pts[b]], [k, k]))
    n = 67
    half = (n + 1) // 2
    ps = [pts[i % len(pts)] for i in range(n)]
    ks = [scalars[(5 * i + 1) % len(scalars)] for i in range(n)]
    for t, (a, b), k in ((0, (0, 1), 1), (1, (2, 3), 1), (2, (0, 1), 3), (half - 2, (2, 3), R + 1)):
        ps[t], ps[t + half], ks[t], ks[t + half] = pts[a], pts[b], k, k
    cases.append((ps, ks))
    try:
        for lat in (LAT_DEFAULT, 0):
            eng.set_latency_threshold(lat)
            for ps, ks in cases:
                want = _osum(group, [_omul(group, p, k) for p, k in zip(ps, ks)])
                got = fn(b"".join(ps), b"".join(k.to_bytes(32, "big") for k in ks), len(ps), any_point=True)
                assert got == want, (NAME[group], lat, len(ps), [hex(k) for k in ks[:2]])
    finally:
        eng.set_latency_threshold(LAT_DEFAULT)


# ---- 6. the lane-pair bucket kernel with a partial-zero pair in one bucket ---------------------------------------------------------------
BUCKET_N = 257


@functools.lru_cache(maxsize=None)
def _bucket_case():
    """257 G2 points for the any-point MSM: two class-d pairs (x agree in c0 only / in c1 only, outside the subgroup), each pair with one scalar
    for both points -- in every window the two fall into the same bucket, where the mixed addition meets a partially zero h -- and copies of
    eight subgroup points under random 256-bit scalars -> (points, scalars, the oracle's sum through the scalar identity)"""
    xs = P.XORShift(9900)
    pools = G.partial_pools()
    dpts = [G.wire(2, a) for a in pools["c0"][0][:2] + pools["c1"][0][:2]]
    base = [G.wire(2, a) for a in G.subgroup_points(2)]
    k1, k2 = P.rand_int(xs, 1 << 255), P.rand_int(xs, 1 << 256)
    pts, ks = [], []
    for i in range(BUCKET_N - 4):
        pts.append(base[i % 8]); ks.append(P.rand_int(xs, 1 << 256))
    col = [sum(k for p, k in zip(pts, ks) if p == b) % R for b in base]
    for at, p, k in ((5, dpts[0], k1), (200, dpts[1], k1), (77, dpts[2], k2), (78, dpts[3], k2)):
        pts.insert(at, p); ks.insert(at, k)
    assert len(pts) == BUCKET_N
    want = _osum(2, [_omul(2, b, c) for b, c in zip(base, col)] + [_omul(2, dpts[0], k1), _omul(2, dpts[1], k1), _omul(2, dpts[2], k2), _omul(2, dpts[3], k2)])
    return b"".join(pts), b"".join(k.to_bytes(32, "big") for k in ks), want


def _bucket_worker():
    from bls_amd import engine as eng
    eng.init(0)
    pts, ks, _ = _bucket_case()
    lib = eng._lib()
    lib.blsmi_set_profiling(1)
    got = eng.g2_msm(pts, ks, BUCKET_N, any_point=True)
    buf = ctypes.create_string_buffer(8192)
    lib.blsmi_last_profile(buf, ctypes.c_size_t(8192)); lib.blsmi_set_profiling(0)
    print("BUCKET_RESULT " + json.dumps({"sum": None if got is None else got.hex(), "profile": buf.value.decode()}), flush=True)


def test_bucket_kernel_with_a_partial_zero_pair_in_one_bucket():
    """BLSMI_MSM_BUCKET_MIN is read at start-up and the bucket method starts at 2^17 points by default: one fresh process with the threshold
    at 257 runs the any-point G2 MSM of _bucket_case through k_g2_msm_bucket_pair (asserted from the profile) to the oracle's sum"""
    env = dict(os.environ)
    env["BLSMI_MSM_BUCKET_MIN"] = str(BUCKET_N)
    for name in ("BLSMI_LAYOUT", "BLSMI_MUL_GENERIC", "BLSMI_MSM_SORT"):
        env.pop(name, None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "bucket-worker"], env=env, capture_output=True, text=True, timeout=600)
    line = [l for l in r.stdout.splitlines() if l.startswith("BUCKET_RESULT ")]
    assert r.returncode == 0 and line, (r.returncode, r.stdout[-1500:], r.stderr[-1500:])
    res = json.loads(line[-1][len("BUCKET_RESULT "):])
    assert "k_g2_msm_bucket_pair" in res["profile"], res["profile"]
    want = _bucket_case()[2]
    assert want is not None and res["sum"] == want.hex()


if __name__ == "__main__":
    assert sys.argv[1:] == ["bucket-worker"], sys.argv
    _bucket_worker()
