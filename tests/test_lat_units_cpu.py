"""CPU (no GPU): the unit programs of the latency path (bls_amd/csrc/gen_lat.py: UNIT_PROGRAMS) -- (a) the generator's exact simulator agrees
with the job kinds' formulas, (b) the SCHEDULED programs hold the job shapes they are there for (the builder materialises operands on its
own: a unit program must not get quietly softer), (c) a limb-exact model of the multiply cores (tests/lat_limb_model.py) stays inside int32 /
int64 at the bounds the builder admits and leaves them one step beyond.

Two shapes one might ask for cannot exist, by the builder's own bounds:
  * a MUL job with 7 terms on BOTH operands: a term has |c| >= 1, so La, Lb >= 7 and La * Lb >= 49 > LPROD_MAX = 33 (15 (La Lb + 1) 2^54 < 2^63,
    fp.cuh).  What the kernel sees of it is a level header with ntx = nty = 7; the programs have levels with a 7 x 4-term and a 4 x 7-term job.
  * a SQR operand with 3 V^2 >= 0.9 VPROD_MAX (V >= 1587): an operand has L <= 2 and a node's value bound is at most V_REDUCE_AT = 512 (a LIN result
    above it is reduced to V = 3), so V <= 1024 and 3 V^2 <= 3 145 728 = 0.375 VPROD_MAX.  (With L <= 3 it was 1536: 0.84.)  The programs go to 1024."""
import pytest

import lat_limb_model as M
import lat_operands as O
import lat_units as U
from oracle import pyref as P

G = U.G
Q = U.Q
MUL_SHAPES = {(1, 1), (1, 15), (15, 2), (2, 15), (3, 11), (11, 3), (4, 8), (8, 4), (5, 6)}


def _jobs(kind):
    for name in G.UNIT_PROGRAMS:
        for li, (k, jobs) in enumerate(U.program(name).levels):
            if k == kind:
                for n in jobs:
                    yield name, li, n


def _levels(kind):
    for name in G.UNIT_PROGRAMS:
        for li, (k, jobs) in enumerate(U.program(name).levels):
            if k == kind:
                yield name, li, jobs


@pytest.mark.parametrize("name", G.UNIT_PROGRAMS)
def test_simulator_equals_the_formulas(name):
    """G.simulate works on field elements (no Montgomery factor): its output times R is the raw value the formulas give"""
    p = U.program(name)
    xs = P.XORShift(77)
    k = U.nin(name)
    rows = [[O.value(e) for e in t] for t in U.tuples(name)[:40:3]] + [[P.rand_int(xs, Q) for _ in range(k)] for _ in range(3)]
    for raw in rows:
        sim = G.simulate(p, {G.BUF_RAW3: [v * U.RINV % Q for v in raw]})
        want = U.evaluate(p, raw)
        assert [s * U.R % Q for s in sim] == [w[1] for w in want]
        assert all(ex is None or ex % Q == v for _, v, ex in want)


def test_programs_are_within_the_image_contract():
    for name in G.UNIT_PROGRAMS:
        p = U.program(name)
        assert len(p.out_nodes) <= 12 and len(p.inputs) == len(G.build_unit_program(name).inputs)        # every input is read
        assert all(n.aux[0] == G.BUF_RAW3 for n in p.inputs) and sorted(n.aux[1] for n in p.inputs) == list(range(len(p.inputs)))
        assert p.out == {"unit_check1": "check1", "unit_iszero": "iszero"}.get(name, "outraw12")
        assert not p.consts
    assert set(G.UNIT_PROGRAMS).isdisjoint(G.SHIPPED_PROGRAMS)


def test_mul_shapes_are_scheduled():
    jobs = list(_jobs(G.K_MUL))
    shapes = {(n.x.L(), n.y.L()) for _, _, n in jobs}
    assert MUL_SHAPES <= shapes and max(a * b for a, b in shapes) == G.LPROD_MAX
    assert not [n for _, _, n in jobs if len(n.x) == 7 and len(n.y) == 7]                     # cannot exist (module docstring)
    assert [n for _, _, n in jobs if len(n.x) == 7 and len(n.y) >= 4] and [n for _, _, n in jobs if len(n.x) >= 4 and len(n.y) == 7]
    coefs = {c for _, _, n in jobs for lin in (n.x, n.y) for c in lin.values()}
    assert coefs == set(range(-15, 16)) - {0}
    assert sum(1 for _, _, n in jobs for lin in (n.x, n.y) if min(lin.values()) < 0 < max(lin.values())) >= 20   # mixed signs inside one gather
    for name, li, lv in _levels(G.K_MUL):
        if name in ("unit_mul0", "unit_mul1", "unit_mul2"):
            assert len({len(n.x) for n in lv}) >= 3 and len({len(n.y) for n in lv}) >= 3      # different term counts in one level
    # ... and as the kernel reads it: the header carries the maximum, the idle term fields are NOTERM
    p = U.program("unit_mul0")
    (h, desc), = [(h, d) for h, d in G.executed_levels(G.encode(p)) if h[0] == G.K_MUL]
    assert (h[1], h[2]) == (7, 7)
    import struct
    noterm = 16 << 11
    for lane, n in enumerate(p.levels[1][1]):
        row = struct.unpack_from("<16H", desc, 32 * lane)
        assert all(f != noterm for f in row[1:1 + len(n.x)]) and all(f == noterm for f in row[1 + len(n.x):8])
        assert all(f != noterm for f in row[8:8 + len(n.y)]) and all(f == noterm for f in row[8 + len(n.y):15])


def test_value_bound_products_are_scheduled():
    big = [n for _, _, n in _jobs(G.K_MUL) if 10 * n.x.V() * n.y.V() >= 9 * G.VPROD_MAX]
    assert len(big) >= 8 and all(n.x.V() * n.y.V() <= G.VPROD_MAX for n in big)
    assert max(n.x.V() * n.y.V() for n in big) == G.VPROD_MAX
    assert max(n.x.L() * n.y.L() for n in big) == G.LPROD_MAX
    assert {(n.x.L(), n.y.L()) for n in big} == {(4, 8), (8, 4), (3, 11), (11, 3)}
    lin_level = {id(n): jobs for _, _, jobs in _levels(G.K_LIN) for n in jobs}
    for n in big:                                                                             # operands: un-reduced LIN results over un-reduced LIN results
        for d in list(n.x) + list(n.y):
            assert d.kind == "lin" and not U.level_reduces(lin_level[id(d)]) and d.V >= 496
            assert any(e.kind == "lin" and not U.level_reduces(lin_level[id(e)]) for e in d.x)


def test_sqr_shapes_are_scheduled():
    jobs = [n for _, _, n in _jobs(G.K_SQR)]
    assert {n.x.L() for n in jobs} == {1, 2} and G.SQR_LMAX == 2
    assert {len(n.x) for n in jobs if n.x.L() == 2} == {1, 2}
    assert {c for n in jobs for c in n.x.values()} == {-2, -1, 1, 2}
    assert max(n.x.V() for n in jobs) == G.SQR_LMAX * G.V_REDUCE_AT == 1024                   # the most the builder admits (module docstring)
    assert sum(1 for n in jobs if n.x.V() == 1024) >= 4


def test_lin_levels_are_scheduled():
    seen = set()
    for name, li, jobs in _levels(G.K_LIN):
        split = 4 if len(jobs) <= 16 else 2 if len(jobs) <= 32 else 1                         # gen_lat.py encode
        seen.add((split, U.level_reduces(jobs)))
    assert seen == {(s, r) for s in (4, 2, 1) for r in (False, True)}
    # ... and as encoded: the lanes-per-job byte and the level-wide reduction bit
    hdrs = {(h[3], bool(h[0] & 0x80)) for name in G.UNIT_PROGRAMS for h, _ in G.executed_levels(G.encode(U.program(name))) if h[0] & 0x7f == G.K_LIN}
    assert hdrs == seen
    jobs = [(name, li, n) for name, li, n in _jobs(G.K_LIN)]
    lv = {(name, li): js for name, li, js in _levels(G.K_LIN)}
    assert sum(1 for _, _, n in jobs if len(n.x) == G.TLIN and n.x.L() == G.LMAX) >= 8
    assert {s for s in (4, 2, 1) for name, li, n in jobs if len(n.x) == G.TLIN and n.x.L() == G.LMAX
            and s == (4 if len(lv[name, li]) <= 16 else 2 if len(lv[name, li]) <= 32 else 1)} == {4, 2, 1}
    unred = [n for name, li, n in jobs if not U.level_reduces(lv[name, li])]
    red = [n for name, li, n in jobs if U.level_reduces(lv[name, li])]
    assert max(n.x.V() for n in unred) == G.V_REDUCE_AT and max(n.x.V() for n in red) == G.LIN_VMAX == 4096
    assert sum(1 for n in red if n.x.V() == G.LIN_VMAX) >= 6
    mixed = [js for js in lv.values() if len({n.reduce for n in js}) == 2]
    assert mixed and U.program("unit_linmix").levels[1][1] in mixed
    assert {c for _, _, n in jobs for c in n.x.values()} == set(range(-15, 16)) - {0}
    # the un-reduced results that leave come from narrow levels of un-reduced jobs only
    for name in G.UNIT_PROGRAMS:
        p = U.program(name)
        for n in p.out_nodes:
            if n.kind == "lin" and not n.reduce and name != "unit_linmix":
                assert not U.level_reduces(p.levels[n.level][1]) and len(p.levels[n.level][1]) <= 16


def test_inv_and_verdict_programs_are_scheduled():
    p = U.program("unit_inv")
    inv = [n for k, jobs in p.levels if k == G.K_INV for n in jobs]
    assert len(inv) == 4
    for n in inv:
        (d, c), = n.x.items()
        assert c == 1 and d.kind == "lin" and d.reduce
    for name in ("unit_check1", "unit_iszero"):
        p = U.program(name)
        assert len(p.out_nodes) == 12 and all(n.kind == "lin" and n.reduce and len(n.x) == 1 for n in p.out_nodes)


# ---- (c) the limb-exact model ----------------------------------------------------------------------------------------------------------
def _extreme(L, pattern):
    """a gathered operand with limbs 0..13 at the bound of L, L (2^27 + 64): L times an extreme-limb input (all plus, all minus, alternating)"""
    e = {"+": O.ALL_PLUS, "-": O.neg(O.ALL_PLUS), "a": O.ALT0}[pattern]
    return M.gather([(L, e)])


def _worst(L, pattern):
    """EVERY limb at L (2^27 + 64), the top one too -- what the limb bound of Fp<L, V> alone admits and fp.cuh's head-room formula
    15 (La Lb + 1) 2^54 < 2^63 is written for (no value within the value bounds has such a top limb)"""
    b = L * O.BOUND
    return [b if pattern == "+" else -b if pattern == "-" else (b if i % 2 == 0 else -b) for i in range(M.NL)]


def _check_product(a, b):
    r, peak = M.lat_mul(a, b)
    assert M.value(r) % Q == M.value(a) * M.value(b) * U.RINV % Q
    assert all(0 <= l < (1 << 27) for l in r[:14])
    return peak


@pytest.mark.parametrize("La,Lb", sorted(MUL_SHAPES))
def test_limb_model_mul_at_the_bounds(La, Lb):
    assert La * Lb <= G.LPROD_MAX
    for pa, pb in (("+", "+"), ("-", "-"), ("+", "-"), ("a", "a"), ("a", "+")):
        peak = _check_product(_extreme(La, pa), _extreme(Lb, pb))
        assert peak < 1 << 63


def test_limb_model_mul_headroom():
    """La * Lb = 33 fits with limbs 0..13 of both operands at their bounds, the accumulator peaking above 2^62.  One step beyond every shape
    (La * Lb >= 35) the formula's worst case -- all 15 limbs at the bound, equal signs -- overflows the accumulator in column 14:
    15 * 35 * (2^27 + 64)^2 > 2^63 whatever the m q terms add.  And L = 16 no longer fits a gathered int32 limb."""
    peaks = [_check_product(_extreme(a, "+"), _extreme(b, "+")) for a, b in ((3, 11), (11, 3))]
    assert all((1 << 62) < p < (1 << 63) for p in peaks)
    for a, b in ((3, 12), (12, 3), (4, 9), (9, 4), (5, 7), (7, 5), (6, 6), (3, 15), (15, 3)):                # one step beyond each shape
        assert a * b > 34
        for pat in (("+", "+"), ("-", "-"), ("a", "a")):
            with pytest.raises(M.Overflow, match="accumulator"):
                M.lat_mul(_worst(a, pat[0]), _worst(b, pat[1]))
    M.gather([(15, O.ALL_PLUS)]); M.gather([(-15, O.ALL_PLUS)])
    M.gather([(c, O.ALL_PLUS if c > 0 else O.neg(O.ALL_PLUS)) for c in (3, -2, 2, -2, 2, -2, 2)])
    with pytest.raises(M.Overflow, match="gathered limb"):                                                  # (1, 16), (2, 16)
        M.gather([(15, O.ALL_PLUS), (1, O.ALL_PLUS)])
    with pytest.raises(M.Overflow, match="gathered limb"):
        M.gather([(-15, O.ALL_PLUS), (1, O.neg(O.ALL_PLUS))])


def test_limb_model_sqr3_at_the_bound_and_beyond():
    """the squaring core forms 6a in int32: exact for L <= 2 (the bound Builder.sqr3 enforces), wrapped at L = 3 for every |limb| > 357 913 941"""
    for L in (1, 2):
        for pat in ("+", "-", "a"):
            a = _extreme(L, pat)
            r, peak = M.lat_sqr3(a)
            assert M.value(r) % Q == 3 * M.value(a) ** 2 * U.RINV % Q and all(0 <= l < (1 << 27) for l in r[:14]) and peak < 1 << 63
    direct = [n for _, _, n in _jobs(G.K_SQR) if all(d.kind == "in" for d in n.x)]      # the unit program's own jobs over inputs, from the job table
    assert len(direct) >= 8
    for t in U.tuples("unit_sqr")[:12]:
        for n in direct:
            a = M.gather([(c, t[d.aux[1]]) for d, c in n.x.items()])
            assert M.value(M.lat_sqr3(a)[0]) % Q == 3 * M.value(a) ** 2 * U.RINV % Q
    assert 6 * 357913941 < (1 << 31) <= 6 * 357913942
    for pat in ("+", "-", "a"):
        a = _extreme(3, pat)
        with pytest.raises(M.Overflow, match="6 a"):
            M.lat_sqr3(a)
        r, _ = M.lat_sqr3(a, wrap6=False)                               # without the int32 store of 6a the same operands square correctly
        assert M.value(r) % Q == 3 * M.value(a) ** 2 * U.RINV % Q
    assert G.SQR_LMAX == 2
    b = G.Builder()
    x = G.Lin({b.inp(G.BUF_RAW3, 0).popitem()[0]: 3})
    (n, c), = b.sqr3(x).items()
    assert n.kind == "sqr3" and n.x.L() == 1                            # an L = 3 operand is materialised first


def test_limb_model_on_the_unit_products():
    """the model on the gathered operands of every MUL unit job, at the sign tuples of the GPU test"""
    for name in ("unit_mul0", "unit_mul1", "unit_mul2"):
        p = U.program(name)
        for t in U.tuples(name)[:12]:
            for n in p.levels[1][1]:
                a = M.gather([(c, t[d.aux[1]]) for d, c in n.x.items()]); b = M.gather([(c, t[d.aux[1]]) for d, c in n.y.items()])
                _check_product(a, b)
