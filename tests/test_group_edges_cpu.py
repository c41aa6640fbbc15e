"""The group-law corpus (tests/group_edges.py) has the properties its labels claim -- h and rr0 computed with big integers from the records
the kernels receive -- and the C oracle agrees with its Python twin on every pair of it: additions, doublings and the segment sums of
tests/test_gpu_group_edges.py.  The GPU tests compare against the C oracle alone; this file is what says the oracle's own special cases
(the same point, opposite points, an infinite operand, a partially zero difference) are the reference's."""
import collections

import numpy as np
import pytest

import group_edges as G
from gpu_common import P, RC

Q = P.Q
GROUPS = (1, 2)
ADD = {1: RC.g1_add, 2: RC.g2_add}
DBL = {1: RC.g1_double, 2: RC.g2_double}
TO_AFF = {1: RC.g1_jac_to_affine_bytes, 2: RC.g2_jac_to_affine_bytes}


def _zero_pattern(group, v):
    """which coefficients of a field element are zero, as a tuple of booleans"""
    return tuple(c % Q == 0 for c in G.coeffs(group, v))


def _from_records(group, pair):
    """the operands as the kernels get them: through the Montgomery records and back"""
    return G.unrecord(group, G.record(group, pair.p)), G.unrecord(group, G.record(group, pair.q))


@pytest.mark.parametrize("group", GROUPS)
def test_corpus_has_the_properties_its_labels_claim(group):
    F = G.FIELD[group]
    n = collections.Counter()
    all_zero, none_zero = (True,) * group, (False,) * group
    for c in G.corpus(group):
        p, q = _from_records(group, c)
        assert (p, q) == (c.p, c.q), c.label
        h, rr0 = G.h_rr0(group, p, q)
        zh, zr = _zero_pattern(group, h), _zero_pattern(group, rr0)
        fin_p, fin_q = p[2] != F.zero, q[2] != F.zero
        key = c.label
        if c.pa is not G.NOT_A_POINT:                                    # the records stand for the affine points they say, and those are curve points
            for jac, a, fin in ((p, c.pa, fin_p), (q, c.qa, fin_q)):
                assert (a is not None) == fin and G.on_curve(group, a), c.label
                assert P.jac_to_affine(F, jac) == a, c.label
        if c.label == "same":
            assert fin_p and fin_q and p[2] != q[2] and zh == all_zero and zr == all_zero
        elif c.label == "opposite":
            assert fin_p and fin_q and p[2] != q[2] and zh == all_zero and rr0 != F.zero
        elif c.label in ("inf_left", "inf_right", "inf_both"):
            assert (fin_p, fin_q) == {"inf_left": (False, True), "inf_right": (True, False), "inf_both": (False, False)}[c.label]
            first = p if not fin_p else q                                # the shape of the (first) infinite operand: (0, 1, 0), or X and Y non-zero
            assert first[:2] == (F.zero, F.one) or (first[0] != F.zero and first[1] != F.zero)
            key += "/01" if first[:2] == (F.zero, F.one) else "/xy"
        elif c.label in ("d_c0", "d_c1"):
            assert zh == ((True, False) if c.label == "d_c0" else (False, True)), (c.label, zh)
            key += "/affine" if p[2] == q[2] == P.FQ2_ONE else "/z"
        elif c.label in ("d_c0_x", "d_c1_x"):
            dx = F.sub(c.qa[0], c.pa[0])
            assert _zero_pattern(2, dx) == ((True, False) if c.label == "d_c0_x" else (False, True))
        elif c.label.startswith("e_y"):
            assert zh == all_zero and zr == ((True, False) if c.label == "e_y_c0" else (False, True)), (c.label, zh, zr)
            key += "/z1" if p[2] == q[2] == P.FQ2_ONE else "/z"
        elif c.label.startswith("e_x"):
            assert zh == ((True, False) if c.label == "e_x_c0" else (False, True)), (c.label, zh)
            key += "/z1" if p[2] == q[2] == P.FQ2_ONE else "/z"
        else:
            assert c.label == "generic" and fin_p and fin_q and zh == none_zero
        n[key] += 1
    assert len(G.corpus(group)) % 2 == 1 and len(G.corpus(group)) > 64
    assert n["same"] >= G.SAME_OPPOSITE_MIN and n["opposite"] >= G.SAME_OPPOSITE_MIN, n
    assert min(n["inf_left/xy"], n["inf_left/01"], n["inf_right/xy"], n["inf_right/01"], n["inf_both/xy"], n["inf_both/01"]) >= 1, n
    if group == 2:
        for kind in ("d_c0", "d_c1"):
            assert n[kind + "/affine"] >= G.PARTIAL_MIN and n[kind + "/z"] >= G.PARTIAL_MIN and n[kind + "_x"] >= G.PARTIAL_MIN, n
        for kind in ("e_y_c0", "e_y_c1", "e_x_c0", "e_x_c1"):
            assert n[kind + "/z1"] >= G.PARTIAL_MIN and n[kind + "/z"] >= G.PARTIAL_MIN, n


@pytest.mark.parametrize("group", GROUPS)
def test_corpus_covers_every_z_value_both_subgroups_and_x_zero(group):
    F = G.FIELD[group]
    same = [c for c in G.corpus(group) if c.label == "same"]
    zs = {c.p[2] for c in same} | {c.q[2] for c in same}
    if group == 1:
        assert set(G.fq_z_values()) <= zs
        assert {(0, 2), (0, Q - 2)} <= {c.pa for c in same}
    else:
        seen = {v for z in zs for v in z}
        assert set(G.fq_z_values()) <= seen and any(z[0] == 0 for z in zs) and any(z[1] == 0 for z in zs)
        xs = {c.pa[0] for c in same}
        assert any(x[0] == 0 and x[1] for x in xs) and any(x[1] == 0 and x[0] for x in xs)
    for v in (1, 2, Q - 1, (Q - 1) // 2, (Q + 1) // 2):
        assert v in G.fq_z_values()
    inside = P.g1_in_subgroup if group == 1 else P.g2_in_subgroup
    assert all(inside(a) for a in G.subgroup_points(group)) and not any(inside(a) for a in G.outside_points(group))
    assert all(G.on_curve(group, a) for a in G.base_points(group))
    labels, ops = G.doubling_operands(group)
    assert len(ops) % 2 == 1 and len(ops) > 64 and "inf" in labels and "same" in labels
    assert sum(1 for p in ops if p[2] == F.zero) >= 3
    if group == 2:
        assert {"d_c0", "d_c1", "e_y_c0", "e_x_c1"} <= set(labels)


def _affine_of_twin(group, jac):
    return G.wire(group, P.jac_to_affine(G.FIELD[group], jac))


@pytest.mark.parametrize("group", GROUPS)
def test_oracle_additions_match_the_python_twin(group):
    """RC.g?_add against pyref.jac_add in both operand orders: equal as affine points and as infinity flags; the crafted records, whose sums
    are no curve points, as raw Jacobian coordinates"""
    F = G.FIELD[group]
    for c in G.corpus(group):
        for p, q in ((c.p, c.q), (c.q, c.p)):
            got = ADD[group](G.record(group, p), G.record(group, q))
            want = P.jac_add(F, p, q)
            assert (TO_AFF[group](got) is None) == P.jac_is_zero(F, want), c.label
            assert TO_AFF[group](got) == _affine_of_twin(group, want), c.label
            if c.pa is G.NOT_A_POINT:
                assert G.unrecord(group, got) == want, c.label


@pytest.mark.parametrize("group", GROUPS)
def test_oracle_doublings_match_the_python_twin(group):
    F = G.FIELD[group]
    labels, ops = G.doubling_operands(group)
    for label, p in zip(labels, ops):
        got = DBL[group](G.record(group, p))
        want = P.jac_double(F, p)
        assert (TO_AFF[group](got) is None) == P.jac_is_zero(F, want), label
        assert TO_AFF[group](got) == _affine_of_twin(group, want), label
        if label.startswith("e_"):
            assert G.unrecord(group, got) == want, label


@pytest.mark.parametrize("group", GROUPS)
def test_oracle_segment_sums_match_a_left_fold_of_the_python_twin(group):
    F = G.FIELD[group]
    case = G.sum_case(group)
    assert len(case.segs) % 2 == 1 and len(case.segs) > 64 and len(case.table) == len(case.jtab) == len(case.inf)
    pts = [None if case.inf[i] else G.unwire(group, case.table[i]) for i in range(len(case.table))]
    for i, j in enumerate(case.jtab):                                    # the in-memory table holds the same points, under Z != 1
        rec = np.frombuffer(j, dtype=np.uint64)
        assert TO_AFF[group](rec) == (None if case.inf[i] else case.table[i]), i
    assert sum(1 for i, j in enumerate(case.jtab) if not case.inf[i] and G.unrecord(group, np.frombuffer(j, dtype=np.uint64))[2] != F.one) > len(pts) // 2
    infinite = 0
    for seg, label in zip(case.segs, case.labels):
        acc = P.jac_zero(F)
        for i in seg:
            acc = P.jac_add(F, acc, P.to_jac(F, pts[i]))
        want = _affine_of_twin(group, acc)
        assert G.oracle_segment_sum(group, case, seg) == want, label
        infinite += want is None
    assert infinite >= G.SAME_OPPOSITE_MIN
