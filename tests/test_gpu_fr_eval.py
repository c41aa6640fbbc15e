"""-m gpu: polynomials in evaluation form evaluated on the device (blsmi 0.21: blsmi_fr_eval_batch[_dev]; k_fr_bary_prod, k_fr_inv,
k_fr_bary_sum), byte for byte against the big-integer model of tests/fr_eval_cases.py (held against Horner's rule in
tests/test_fr_eval_cpu.py), in both orders and both forms.  Shapes: N = 1, N = 2, N = 32 (most lanes idle), N = 256 (one value per lane),
512 (two), 4 096 and 65 536; one polynomial, a few, and more than one workgroup's worth of inversions' lanes (70)."""
import random

import numpy as np
import pytest

from fr_eval_cases import R, TOP, domain, evaluate, is_noncanon, poly_bytes, second_representatives
from kzg_cases import scalar_bytes
from test_gpu_pprod_rlc import _t
from test_gpu_pprod_rlc_segments import _segments

pytestmark = pytest.mark.gpu

SHAPES = [(0, 3), (1, 3), (5, 1), (5, 3), (5, 70), (8, 1), (8, 3), (8, 70), (9, 3), (12, 3), (16, 1)]   # (log2n, m)
EDGE_VALUES = (0, R - 1, R, TOP)


@pytest.fixture(scope="module")
def eng():
    from bls_amd import engine
    engine.init(0)
    return engine


@pytest.fixture(scope="module")
def fr(eng):
    from bls_amd import fr
    return fr


def root_positions(k):
    """position 0, position N - 1, one in lane 255's share and one in the last wave (lanes 192 .. 255) where N reaches them"""
    n = 1 << k
    return sorted({0, n - 1} | ({255 + 256 * (n // 512), 200} if n >= 256 else set()))


def points(k, order, rng):
    """the points a shape is run at: random ones, the ends of the range, and roots in every 256-bit representative"""
    dom = domain(k, order)
    out = [rng.randrange(R), rng.getrandbits(256), 0, R - 1, R, TOP]
    for pos in root_positions(k):
        out += [dom[pos]] + second_representatives(dom[pos])
    return out


def polynomial(kind, k, order, rng):
    n = 1 << k
    if kind == 0:
        return [rng.randrange(R) for _ in range(n)]
    if kind == 1:
        return [rng.randrange(R)] * n                                            # constant: y = c for every z
    if kind == 2:
        return list(domain(k, order))                                            # f_i = w_i: y = z mod r
    f = [rng.getrandbits(256) if i % 5 == 0 else rng.randrange(R) for i in range(n)]
    for i, v in zip(rng.sample(range(n), min(n, 4)), EDGE_VALUES):               # 0, r - 1, r and 2^256 - 1 mixed in
        f[i] = v
    return f


@pytest.fixture(scope="module")
def batches():
    """{(k, order, m): (polys, zs, expected y, expected noncanon)}, the model computed once"""
    out = {}
    for k, m in SHAPES:
        for order in (0, 1):
            rng = random.Random(1000 * k + 10 * m + order)
            pts = points(k, order, rng)
            polys = [polynomial(j % 4, k, order, rng) for j in range(m)]
            zs = [pts[(j + (j // len(pts))) % len(pts)] if m > 1 else pts[0] for j in range(m)]
            out[(k, order, m)] = (polys, zs, [evaluate(f, k, order, z) for f, z in zip(polys, zs)], [is_noncanon(f) for f in polys])
    return out


def _ints(y):
    return [int.from_bytes(bytes(row), "big") for row in np.asarray(y).reshape(-1, 32)]


@pytest.mark.parametrize("k,m", SHAPES)
def test_against_the_model_in_both_orders_and_forms(fr, batches, k, m):
    import torch
    for order in (0, 1):
        polys, zs, want, want_nc = batches[(k, order, m)]
        pb, zb = poly_bytes(polys), scalar_bytes(zs)
        y, nc = fr.eval_batch(pb, k, zb, order=order)
        assert _ints(y) == want and nc.tolist() == want_nc, (k, order, m)
        y, nc = fr.eval_batch(pb, k, zb, order=order, noncanon=False)            # NULL for noncanon
        assert _ints(y) == want and nc is None, (k, order, m)
        dp, dz = _t(pb), _t(zb)
        keep = (dp.clone(), dz.clone())
        st = torch.cuda.Stream(device=dp.device)
        for d_nc, stream in ((True, 0), (False, st.cuda_stream)):
            dy = torch.full((32 * m + 32,), 0xa5, dtype=torch.uint8, device=dp.device)
            dn = torch.full((m + 4,), 7, dtype=torch.uint8, device=dp.device)
            fr.eval_batch_dev(dp.data_ptr(), k, order, dz.data_ptr(), dy.data_ptr(), dn.data_ptr() if d_nc else 0, m, stream=stream)
            assert _ints(dy[:32 * m].cpu().numpy()) == want and bytes(dy[32 * m:].cpu().numpy()) == b"\xa5" * 32, (k, order, m)
            assert dn.cpu().numpy().tolist() == ([int(v) for v in want_nc] if d_nc else [7] * m) + [7] * 4, (k, order, m)
        assert torch.equal(dp, keep[0]) and torch.equal(dz, keep[1])             # the inputs stay untouched


def test_the_batches_hold_what_they_should(batches):
    """the corpus itself: every kind of polynomial, flagged and unflagged ones, and hits on every root position in every representative"""
    for (k, order, m), (polys, zs, want, want_nc) in batches.items():
        dom = domain(k, order)
        assert all(v < R for v in want)
        if m >= 3:
            assert want[1] == polys[1][0] and (k == 0 or want[2] == zs[2] % R), (k, order, m)   # the constant, and f_i = w_i (N = 1: a constant too)
        if m == 70:
            hits = {(dom.index(z % R), z // R) for z in zs if z % R in dom}
            assert {p for p, _ in hits} >= set(root_positions(k)) and {t for _, t in hits} == {0, 1, 2}, (k, order)
            assert any(want_nc) and not all(want_nc) and {z for z in zs if z % R not in dom} >= {0, R, TOP} and R - 1 in dom, (k, order)   # (-1 is a root)
    assert root_positions(8) == [0, 200, 255] and root_positions(12) == [0, 200, 2303, 4095] and 2303 % 256 == 255 and 192 <= 200 % 256


@pytest.mark.parametrize("order", [0, 1])
def test_every_lagrange_basis_vector(fr, order):
    """f = e_i for each of the N = 32 positions, one fixed z: y is the i-th basis polynomial's value there.  A wrong position-to-root mapping or a
    wrong bit reversal shows here and nowhere else."""
    k, n, z = 5, 32, 0x1234567890abcdef1234567890abcdef
    dom = domain(k, order)
    polys = [[int(i == j) for i in range(n)] for j in range(n)]
    want = [(pow(z, n, R) - 1) * pow(n, -1, R) * dom[j] * pow(z - dom[j], -1, R) % R for j in range(n)]
    assert want == [evaluate(f, k, order, z) for f in polys] and len(set(want)) == n and sum(want) % R == 1
    y, nc = fr.eval_batch(poly_bytes(polys), k, scalar_bytes([z] * n), order=order)
    assert _ints(y) == want and not nc.any()


@pytest.mark.parametrize("k", [5, 8, 9])
def test_hits_and_misses_alternate(fr, k):
    """even polynomials sit on a root (walking through the positions and the representatives), odd ones beside one: z = w_i + 1"""
    rng = random.Random(k)
    for order in (0, 1):
        dom = domain(k, order)
        n, m = 1 << k, 24
        polys = [polynomial(j % 4, k, order, rng) for j in range(m)]
        pos = [(37 * j + (j % 3) * 255) % n for j in range(m)]
        zs = [([dom[p]] + second_representatives(dom[p]))[(j // 2) % 3 % (1 + len(second_representatives(dom[p])))] if j % 2 == 0 else dom[p] + 1 for j, p in enumerate(pos)]
        want = [evaluate(f, k, order, z) for f, z in zip(polys, zs)]
        assert all(want[j] == polys[j][pos[j]] % R for j in range(0, m, 2))
        y, nc = fr.eval_batch(poly_bytes(polys), k, scalar_bytes(zs), order=order)
        assert _ints(y) == want and nc.tolist() == [is_noncanon(f) for f in polys], (k, order)


def test_polys_that_are_only_word_aligned(fr, batches):
    """a device buffer of polynomials 4 bytes off a 16-byte boundary is read byte by byte: the same values"""
    for key in ((8, 1, 3), (9, 0, 3)):
        polys, zs, want, want_nc = batches[key]
        k, order, m = key
        pb = poly_bytes(polys)
        whole = _t(b"\xa5" * 4 + pb + b"\xa5" * 12)
        dp = whole[4:4 + len(pb)]
        assert dp.data_ptr() % 16 == 4
        zw = _t(b"\xa5" * 4 + scalar_bytes(zs) + b"\xa5" * 12)
        yw = _t(b"\xa5" * (4 + 32 * m + 12))
        dn = _t(bytes(m))
        keep = whole.clone()
        fr.eval_batch_dev(dp.data_ptr(), k, order, zw[4:].data_ptr(), yw[4:].data_ptr(), dn.data_ptr(), m)
        got = yw.cpu().numpy()
        assert _ints(got[4:4 + 32 * m]) == want and bytes(got[:4]) == b"\xa5" * 4 and bytes(got[4 + 32 * m:]) == b"\xa5" * 12
        assert dn.cpu().numpy().tolist()[:m] == [int(v) for v in want_nc]
        import torch
        assert torch.equal(whole, keep)


def test_three_launches_whatever_m(eng, fr, batches):
    """with profiling on a call names k_fr_bary_prod, k_fr_inv, k_fr_bary_sum once each, in that order, for one polynomial and for 70 alike"""
    for key in ((5, 1, 1), (5, 1, 70), (8, 0, 70)):
        polys, zs, want, _ = batches[key]
        (y, _), names = _segments(eng, lambda: fr.eval_batch(poly_bytes(polys), key[0], scalar_bytes(zs), order=key[1]))
        assert _ints(y) == want
        assert [n for n in names if n.startswith("k_")] == ["k_fr_bary_prod", "k_fr_inv", "k_fr_bary_sum"], (key, names)
