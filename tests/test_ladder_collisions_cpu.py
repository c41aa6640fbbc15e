"""The integer model of the ladders' additions (tests/ladder_model.py) and the scalars it finds for which a ladder's accumulator meets the
table entry it is about to add.  tests/test_gpu_ladder_collisions.py runs those scalars through the kernels; this file says the model is
sound -- every trace ends at k mod r -- and that each corpus scalar does what its label claims.  No GPU."""
import random

import pytest

import group_edges as G
import ladder_model as L
from gpu_common import P

R, Z = L.R, L.Z
# the scalars of tests/test_gpu_round3.py::test_endomorphism_scalar_multiplication_edge_scalars
EDGE_SCALARS = [0, 1, 2, Z - 1, Z, Z + 1, Z**2 - 1, Z**2, Z**2 + 1, Z**3 - 1, Z**3, Z**3 + 1, R - 1, R, R + 1, 2 * R, (1 << 128) - 1, 1 << 128,
                (1 << 129) - 1, (1 << 255) - 1, 1 << 255, (1 << 256) - 1, (1 << 256) - Z**2, int("01" * 32, 16)]
# what the search by hand behind this corpus had found: the corpus holds at least these
AT_LEAST = {
    "glv_g1": [("same", (0, 1), R + 2 * Z**2), ("same", (0, 1), 2 * R + 4 * Z**2)],
    "glv_g2": [("same", (0, 2), R + 2 * Z**2), ("same", (0, 2), 2 * R + 4 * Z**2), ("same", (0, 3), R + 2 * Z**3), ("same", (0, 3), 2 * R + 2 * Z**3)],
    "plain4": [("same", 63, R + 30), ("same", 63, 2 * R + 28)],
    "fixed_lane": [("same", 31, 2 * (0x74 << 248) - R)],
}


@pytest.mark.parametrize("ladder", L.LADDERS)
def test_every_trace_ends_at_the_scalar_mod_r(ladder):
    rnd = random.Random(4101)
    ks = EDGE_SCALARS + L.scalars(ladder) + [rnd.getrandbits(256) for _ in range(500)] + [rnd.randrange(R) for _ in range(500)]
    for k in ks:
        t = L.TRACE[ladder](k)
        assert t.result == k % R, (ladder, hex(k))
        assert all(0 <= a < R and 0 <= b < R for _, a, b in t.adds)


def test_the_number_of_additions_is_the_schedule_s():
    k = (1 << 256) - 1
    assert len(L.glv(1, k).adds) == 26 * 2 and len(L.glv(2, k).adds) == 14 * 4
    assert len(L.plain4(k).adds) == 64 and len(L.fixed_lane(k).adds) == 32 and len(L.fixed_wave(k).adds) == 5 * 32
    assert len(L.lat_mul(1, k).adds) == 33 + 32 and len(L.lat_mul(2, k).adds) == 3 * 17 + 16


@pytest.mark.parametrize("ladder", L.LADDERS)
def test_every_corpus_scalar_has_the_event_its_label_claims(ladder):
    corpus = L.corpus(ladder)
    kinds = {e.kind for e in corpus}
    assert {"opposite"} <= kinds, ladder
    for e in corpus:
        assert 0 < e.k < 1 << 256
        adds = dict((step, (a, b)) for step, a, b in L.TRACE[ladder](e.k).adds)
        acc, add = adds[e.step]                                        # straight from the additions, not through events_of
        assert acc and add and (acc == add if e.kind == "same" else acc + add == R), e
    # the control of every ladder: k = r and k = 2 r end in opposite points at the last addition
    for k in (R, 2 * R):
        assert [e.kind for e in corpus if e.k == k] == ["opposite"], (ladder, hex(k))
    for kind, step, k in AT_LEAST.get(ladder, []):
        assert L.Entry(ladder, kind, step, k) in corpus, (ladder, kind, step, hex(k))


def test_where_the_events_are_and_how_many():
    """every event is at the LAST addition that involves the accumulator (ladder_model's docstring says why), and the corpus is what the
    enumeration gives: a change of either shows here"""
    last = {"glv_g1": {(0, 1)}, "glv_g2": {(0, 2), (0, 3)}, "plain4": {63}, "fixed_lane": {31}, "fixed_wave": {(1, 0)},
            "lat_mul1": {(0, "R+U")}, "lat_mul2": {(0, "R+U")}}
    same = {}
    for ladder in L.LADDERS:
        assert {e.step for e in L.corpus(ladder)} == last[ladder], ladder
        same[ladder] = len(L.scalars(ladder, "same"))
        assert L.scalars(ladder, "opposite") == [R, 2 * R]
    # G2, stream 2: the last digit e of stream 3 is free, k = m r + 2 m z^2 + e z^3 collides for every e (32 values each for m = 1, 2).
    # fixed_wave DOES have same-point scalars: at the last level lane 0 adds B (the bytes at odd places) to A (those at even places), and
    # B = A + m r has a solution with A + B < 2^256 for m = 1 and for m = 2 (ladder_model._solve_supported), two scalars in all.
    assert same == {"glv_g1": 2, "glv_g2": 66, "plain4": 2, "fixed_lane": 2, "fixed_wave": 2, "lat_mul1": 2, "lat_mul2": 2}


def test_a_sample_of_scalars_below_r_has_no_event():
    """Below r the sub-scalars are the canonical ones and no accumulator meets its addend: 20 000 seeded scalars, every ladder.  A sample,
    not a proof -- the argument is in ladder_model's docstring."""
    rnd = random.Random(4102)
    for _ in range(20000):
        k = rnd.randrange(R)
        for ladder in L.LADDERS:
            assert not L.TRACE[ladder](k).events, (ladder, hex(k))


def test_the_plain_ladder_s_table():
    """tab[2] = P + P is a doubling for every point; a point of order below 16 has infinity in its table, and entries that repeat"""
    assert L.plain4_table().events == [("same", 2)]
    for ell in (3, 11, 13):
        t = L.plain4_table(ell)
        res = [(a + b) % ell for _, a, b in t.adds]
        assert 0 in res and len(set(res)) < len(res) and ("opposite", ell) in t.events
    t = L.plain4_table(23)
    assert t.events == [("same", 2)] and len({(a + b) % 23 for _, a, b in t.adds}) == 14
    # order 23: no infinity in the table, yet the ladder itself collides for ordinary scalars
    rnd = random.Random(4103)
    assert sum(bool(L.plain4(rnd.getrandbits(256), 23).events) for _ in range(100)) > 50


@pytest.mark.parametrize("group,ell", [(g, ell) for g in (1, 2) for ell in G.LOW_ORDERS[g]])
def test_low_order_points(group, ell):
    """by the Python oracle alone: on the curve, finite, [ell] P at infinity"""
    F = G.FIELD[group]
    pt = G.low_order_point(group, ell)
    assert pt is not None and G.on_curve(group, pt)
    assert P.jac_to_affine(F, P.affine_mul(F, pt, ell)) is None
    assert P.jac_to_affine(F, P.affine_mul(F, pt, ell + 1)) == pt
    assert G.CURVE_ORDER[group] % ell == 0 and not (P.g1_in_subgroup(pt) if group == 1 else P.g2_in_subgroup(pt))
    if (group, ell) == (1, 3):
        assert pt in G.x_zero_points(1)                                  # the order-3 points are the x = 0 points the suite already had
