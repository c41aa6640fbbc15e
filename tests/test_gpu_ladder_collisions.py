"""-m gpu: every scalar-multiplication ladder on the scalars for which its own accumulator meets the table entry it is about to add
(tests/ladder_model.py finds them, tests/test_ladder_collisions_cpu.py checks the model): the "same point, so double" and the "opposite
points, so infinity" branches of jac_add_affine_i / jac_add_i INSIDE the register-resident ladders, byte for byte against the C oracle's
bit-serial MulFR, infinity flag included.  Every case asserts from blsmi_last_profile that the intended kernel ran.

  g?_mul_batch           default -> k_lat:mul1 / k_lat:mul2; latency threshold 0 -> k_g1_mul_glv / k_g2_mul_glv_pair; any_point ->
                         k_g1_mul / k_g2_mul_pair
  g?_mul_generator_batch[_jac]   k_g?_mul_fixed_wave (a wave per scalar: n = 1 and n = 3), latency threshold 0 -> k_g?_mul_fixed
  g1_mul_add_batch       k_g1_mul_add_glv: the corpus as z with C random, and C = +-[z] pi, C infinite right after the collision
  g?_msm, n = 67         below the bucket method: the multiples of either path, then their sum
  BLSMI_LAYOUT=single    one fresh child process (the switch is read at start-up): the one-lane k_g2_mul_glv and k_g2_mul
  low-order points       any_point: a G1 point of order 11 (and the order-3 points), twist points of order 13 and 23 -- the table
                         tab[1..15] of the plain ladder then holds infinity and repeats (11, 13) or the ladder collides all the way (23)

Shapes.  sparse: n = 67 (a full and a ragged one-lane workgroup, three lane-pair workgroups), random subgroup points, the corpus at rows
0, 31, 32, 33, 63, 64, 66, r + 1 at row 1, random scalars everywhere else: a collision lane next to ordinary ones in the same wave.  dense:
n = 65, distinct points, rows 0 .. 62 the corpus cycled, rows 63, 64 the controls r + 1 and a random scalar.  alone: n = 1 for each corpus
scalar.  A ladder's batches hold its OWN corpus; the corpus of G2's endomorphism ladder has 68 scalars, of which dense takes the first 63
in the round-robin order of _ordered (every kind and step first) and alone takes all."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":                                                   # the child process of test_one_lane_g2_ladders: python tests/<this file>
    sys.path.insert(0, ROOT)

import group_edges as G
import ladder_model as L
from gpu_common import P, RC, rand_g1, rand_g2
from test_gpu_launch_table import names_of

pytestmark = pytest.mark.gpu

R = L.R
TOP = 1 << 256
GROUPS = (1, 2)
PB = {1: 96, 2: 192}
OMUL = {1: RC.g1_mul, 2: RC.g2_mul}
OSUM = {1: RC.g1_sum, 2: RC.g2_sum}
TO_AFF = {1: RC.g1_jac_to_affine_bytes, 2: RC.g2_jac_to_affine_bytes}
LAT_DEFAULT = 8192
CHILD_LIMIT_S = 300
B = "(between)"
N_SPARSE, N_DENSE = 67, 65
SLOTS = (0, 31, 32, 33, 63, 64, 66)
SHAPES = ("sparse", "dense", "alone")
LADDER = {("lat", 1): "lat_mul1", ("lat", 2): "lat_mul2", ("glv", 1): "glv_g1", ("glv", 2): "glv_g2", ("plain", 1): "plain4", ("plain", 2): "plain4",
          ("wave", 1): "fixed_wave", ("wave", 2): "fixed_wave", ("lane", 1): "fixed_lane", ("lane", 2): "fixed_lane"}
NAMES = {("lat", 1): ["k_lat:mul1", B], ("lat", 2): ["k_lat:mul2", B], ("glv", 1): ["k_g1_mul_glv", B], ("glv", 2): ["k_g2_mul_glv_pair", B],
         ("plain", 1): ["k_g1_mul", B], ("plain", 2): ["k_g2_mul_pair", B],
         ("wave", 1): ["k_g1_mul_fixed_wave", B], ("wave", 2): ["k_g2_mul_fixed_wave", B], ("lane", 1): ["k_g1_mul_fixed", B], ("lane", 2): ["k_g2_mul_fixed", B]}
SINGLE_NAMES = {"glv": ["k_g2_mul_glv", B], "plain": ["k_g2_mul", B]}
MSM_NAMES = {("lat", 1): ["k_lat:mul1", B, "k_lat:sum", B], ("lat", 2): ["k_lat:mul2", B, "k_lat:sum", B],
             ("glv", 1): ["k_g1_mul_glv", B, "k_g1_sum0", "k_g1_sum", "k_g1_sum_final", B],
             ("glv", 2): ["k_g2_mul_glv_pair", B, "k_g2_sum0", "k_g2_sum", "k_g2_sum_final", B]}


# ---- scalars, points, the oracle ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ordered(ladder):
    """the ladder's corpus scalars, the classes (kind, step) taken in turn: any four in a row hold a same-point and an opposite-points one"""
    classes = {}
    for e in L.corpus(ladder):
        classes.setdefault((e.kind, e.step), []).append(e.k)
    lists = [sorted(set(v)) for _, v in sorted(classes.items(), key=str)]
    out = []
    for i in range(max(len(v) for v in lists)):
        out += [v[i] for v in lists if i < len(v)]
    assert {e.kind for e in L.corpus(ladder) if e.k in out[:4]} == {"same", "opposite"}
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _points(group):
    xs = P.XORShift(4200 + group)
    pts = tuple((rand_g1 if group == 1 else rand_g2)(xs) for _ in range(N_SPARSE))
    assert len(set(pts)) == N_SPARSE
    return pts


@functools.lru_cache(maxsize=None)
def _random_scalars(n=N_SPARSE, seed=4210):
    xs = P.XORShift(seed)
    return tuple(P.rand_int(xs, TOP) for _ in range(n))


@functools.lru_cache(maxsize=None)
def _batch(ladder, shape):
    """-> the scalars of one batch (alone: one batch per corpus scalar, see _batches)"""
    ks, rnd = _ordered(ladder), _random_scalars()
    if shape == "sparse":
        out = list(rnd)
        for i, row in enumerate(SLOTS):
            out[row] = ks[i % len(ks)]
        out[1] = R + 1
        return tuple(out)
    return tuple(ks[i % len(ks)] for i in range(N_DENSE - 2)) + (R + 1, rnd[2])


def _batches(ladder, shape):
    """-> [(first point index, scalars)]"""
    if shape == "alone":
        return [(i % N_SPARSE, (k,)) for i, k in enumerate(_ordered(ladder))]
    return [(0, _batch(ladder, shape))]


_MUL = {}


def _omul(group, w, k):
    """the oracle's multiple k * point -> wire bytes or None, cached (every RC.g?_mul of this file goes through here)"""
    key = (group, w, k)
    if key not in _MUL:
        _MUL[key] = OMUL[group](w, k.to_bytes(32, "big"))
    return _MUL[key]


def _kb(ks):
    return b"".join(k.to_bytes(32, "big") for k in ks)


def _bad_rows(group, pts, ks, out, inf):
    """rows that differ from the oracle: the bytes, or the infinity flag (an infinite result is the all-zero record with its flag set)"""
    bad = []
    for i, (p, k) in enumerate(zip(pts, ks)):
        w = _omul(group, p, k)
        if bool(inf[i]) != (w is None) or bytes(out[i]) != (bytes(PB[group]) if w is None else w):
            bad.append((i, hex(k)))
    return bad


def _bad_rows_jac(group, pts, ks, recs):
    """the same for in-memory records: the affine point, and Z exactly zero where the oracle says infinity"""
    w64 = PB[group] // 16 * 3
    bad = []
    for i, (p, k) in enumerate(zip(pts, ks)):
        rec = np.frombuffer(bytes(recs[i]), dtype=np.uint64)
        want = _omul(group, p, k)
        if TO_AFF[group](rec) != want or (want is None and rec[2 * w64 // 3:].any()):
            bad.append((i, hex(k)))
    return bad


@pytest.fixture(scope="module")
def eng():
    from bls_amd import engine
    engine.init(0)
    yield engine
    engine.set_latency_threshold(LAT_DEFAULT)


@pytest.fixture
def lanes(eng):
    """-> a function that takes the latency path away (threshold 0); the default comes back after the test"""
    yield lambda: eng.set_latency_threshold(0)
    eng.set_latency_threshold(LAT_DEFAULT)


# ---- 1. g?_mul_batch: the level programs, the endomorphism ladders, the plain ladder -------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("path", ["lat", "glv", "plain"])
@pytest.mark.parametrize("group", GROUPS)
def test_mul(eng, lanes, group, path, shape):
    fn = eng.g1_mul_batch if group == 1 else eng.g2_mul_batch
    if path != "lat":
        lanes()
    for first, ks in _batches(LADDER[path, group], shape):
        n = len(ks)
        pts = _points(group)[first:first + n]
        (out, inf), names = names_of(eng, lambda: fn(b"".join(pts), _kb(ks), n, any_point=path == "plain"))
        assert names == NAMES[path, group], (group, path, shape, names)
        bad = _bad_rows(group, pts, ks, out, inf)
        assert not bad, (group, path, shape, first, bad[:8])


# ---- 2. PrivToPub over the fixed-base tables ---------------------------------------------------------------------------------------------
def _generator_batches(path):
    ladder = LADDER[path, 1]
    ks = _ordered(ladder)
    if path == "lane":
        return [b[1] for s in SHAPES for b in _batches(ladder, s)]
    # a wave per scalar: each corpus scalar alone, and triples (same, opposite, control) with the same-point scalar at each of the three places
    same, opp, ctl = L.scalars(ladder, "same"), L.scalars(ladder, "opposite"), (R + 1, _random_scalars()[3])
    out = [(k,) for k in ks]
    for i, s in enumerate(same * 3):
        t = [opp[i % 2], ctl[i % 2]]
        t.insert(i % 3, s)
        out.append(tuple(t))
    return out


@pytest.mark.parametrize("jac", [False, True], ids=["affine", "jac"])
@pytest.mark.parametrize("path", ["wave", "lane"])
@pytest.mark.parametrize("group", GROUPS)
def test_mul_generator(eng, lanes, group, path, jac):
    gen = RC.g1_generator() if group == 1 else RC.g2_generator()
    if path == "lane":
        lanes()
    sizes = set()
    for ks in _generator_batches(path):
        n = len(ks)
        sizes.add(n)
        if jac:
            fn = eng.g1_mul_generator_batch_jac if group == 1 else eng.g2_mul_generator_batch_jac
            recs, names = names_of(eng, lambda: fn(_kb(ks), n))
            bad = _bad_rows_jac(group, [gen] * n, ks, recs)
        else:
            fn = eng.g1_mul_generator_batch if group == 1 else eng.g2_mul_generator_batch
            (out, inf), names = names_of(eng, lambda: fn(_kb(ks), n))
            bad = _bad_rows(group, [gen] * n, ks, out, inf)
        assert names == NAMES[path, group], (group, path, n, names)
        assert not bad, (group, path, jac, n, bad[:8])
    assert sizes == ({1, 3} if path == "wave" else {1, N_DENSE, N_SPARSE})


# ---- 3. out = A + [k] B: the ladder's collision, then an exceptional final addition -------------------------------------------------------
def _mul_add_cases():
    """-> [(rows of (A, B, k))]: the three shapes with A random, and per corpus scalar (and control) A = [k] B (the final addition doubles;
    for k = r, 2 r both operands are infinite), A = -[k] B (infinity) and A infinite -- a batch of their own, and each row alone"""
    from kzg_cases import INF, g1_mul, g1_neg
    pts, other = _points(1), _points(1)[::-1]
    cases = []
    for shape in SHAPES:
        for first, ks in _batches("glv_g1", shape):
            cases.append([(other[(first + i) % N_SPARSE], pts[first + i], k) for i, k in enumerate(ks)])
    rows = []
    for i, k in enumerate(_ordered("glv_g1") + (R + 1, _random_scalars()[4])):
        b = pts[i]
        kb = g1_mul(b, k)
        rows += [(kb, b, k), (g1_neg(kb), b, k), (INF, b, k)]
    cases.append(rows)
    cases += [[r] for r in rows]
    return cases


def test_g1_mul_add(eng):
    from bls_amd import kzg
    from kzg_cases import INF, g1_mul, g1_sum
    eng.set_latency_threshold(LAT_DEFAULT)
    for rows in _mul_add_cases():
        n = len(rows)
        want = [g1_sum([a, g1_mul(b, k)]) for a, b, k in rows]
        (out, inf), names = names_of(eng, lambda: kzg.g1_mul_add_batch(b"".join(a for a, _, _ in rows), b"".join(b for _, b, _ in rows), _kb([k for _, _, k in rows]), n))
        assert names[:1] == ["k_g1_mul_add_glv"], names
        got = [bytes(r) for r in np.asarray(out, dtype=np.uint8).reshape(-1, 96)]
        bad = [(i, hex(rows[i][2])) for i in range(n) if got[i] != want[i] or bool(inf[i]) != (want[i] == INF)]
        assert not bad, (n, bad[:8])


# ---- 4. a small MSM whose scalars are the corpus -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["lat", "glv"])
@pytest.mark.parametrize("group", GROUPS)
def test_msm_below_the_bucket_method(eng, lanes, group, path):
    fn = eng.g1_msm if group == 1 else eng.g2_msm
    if path == "glv":
        lanes()
    pts, ks = _points(group), _batch(LADDER[path, group], "sparse")
    got, names = names_of(eng, lambda: fn(b"".join(pts), _kb(ks), N_SPARSE))
    assert names == MSM_NAMES[path, group], names
    multiples = [w for w in (_omul(group, p, k) for p, k in zip(pts, ks)) if w is not None]
    assert len(multiples) < N_SPARSE                                         # (the opposite-points rows are infinite)
    assert got == OSUM[group](b"".join(multiples), len(multiples))


# ---- 5. points of low order on the plain ladder --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _low_order_items(group):
    """-> ((point, scalar), ...): every low-order point of the group under 0, 1, l - 1, l, l + 1, 15, 16, 17, 2 l, r, 2^256 - 1 and three random
    scalars; a subgroup point between them as the control"""
    xs = P.XORShift(4300 + group)
    items = []
    for ell in G.LOW_ORDERS[group]:
        w = G.wire(group, G.low_order_point(group, ell))
        ks = [0, 1, ell - 1, ell, ell + 1, 15, 16, 17, 2 * ell, R, TOP - 1] + [P.rand_int(xs, TOP) for _ in range(3)]
        items += [(w, k) for k in ks] + [(_points(group)[ell], R + ell)]
    return tuple(items)


@pytest.mark.parametrize("group", GROUPS)
def test_low_order_points_on_the_plain_ladder(eng, group):
    items = _low_order_items(group)
    n = len(items)
    assert n <= 70
    fn = eng.g1_mul_batch if group == 1 else eng.g2_mul_batch
    pts, ks = [p for p, _ in items], [k for _, k in items]
    (out, inf), names = names_of(eng, lambda: fn(b"".join(pts), _kb(ks), n, any_point=True))
    assert names == NAMES["plain", group], names
    bad = _bad_rows(group, pts, ks, out, inf)
    assert not bad, (group, bad[:8])
    assert sum(bool(f) for f in inf) >= 3 * len(G.LOW_ORDERS[group])          # k = 0, l, 2 l of every point


# ---- 6. BLSMI_LAYOUT=single: the one-lane G2 ladders ----------------------------------------------------------------------------------------
def _single_cases():
    """-> [(label, path, points, scalars)] for the child: the endomorphism ladder and the plain ladder on the sparse and the dense batch,
    three corpus scalars alone, and the low-order items on the plain ladder"""
    cases = []
    for path in ("glv", "plain"):
        ladder = LADDER[path, 2]
        for shape in ("sparse", "dense"):
            ks = _batch(ladder, shape)
            cases.append((path + "/" + shape, path, _points(2)[:len(ks)], ks))
        for i, k in enumerate(_ordered(ladder)[:3]):
            cases.append(("%s/alone%d" % (path, i), path, _points(2)[i:i + 1], (k,)))
    items = _low_order_items(2)
    cases.append(("plain/low-order", "plain", tuple(p for p, _ in items), tuple(k for _, k in items)))
    return cases


def _single_worker():
    from bls_amd import engine as eng
    eng.init(0)
    eng.set_latency_threshold(0)
    res = {}
    for label, path, pts, ks in _single_cases():
        (out, inf), names = names_of(eng, lambda: eng.g2_mul_batch(b"".join(pts), _kb(ks), len(ks), any_point=path == "plain"))
        res[label] = {"names": names, "out": [bytes(r).hex() for r in out], "inf": [int(bool(f)) for f in inf]}
    print("SINGLE_RESULT " + json.dumps(res), flush=True)


def test_one_lane_g2_ladders():
    """the one-lane k_g2_mul_glv and k_g2_mul run only under BLSMI_LAYOUT=single, which is read at start-up: one fresh process runs
    _single_cases and sends the records back; the comparison with the oracle is here"""
    env = dict(os.environ, BLSMI_LAYOUT="single")
    for name in ("BLSMI_MUL_GENERIC", "BLSMI_MSM_BUCKET_MIN"):
        env.pop(name, None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "single-worker"], env=env, capture_output=True, text=True, timeout=CHILD_LIMIT_S)   # a new process, never exec
    line = [l for l in r.stdout.splitlines() if l.startswith("SINGLE_RESULT ")]
    assert r.returncode == 0 and line, (r.returncode, r.stdout[-1500:], r.stderr[-1500:])
    res = json.loads(line[-1][len("SINGLE_RESULT "):])
    for label, path, pts, ks in _single_cases():
        got = res[label]
        assert got["names"] == SINGLE_NAMES[path], (label, got["names"])
        bad = _bad_rows(2, pts, ks, [bytes.fromhex(h) for h in got["out"]], got["inf"])
        assert not bad, (label, bad[:8])


if __name__ == "__main__":
    assert sys.argv[1:] == ["single-worker"], sys.argv
    _single_worker()
