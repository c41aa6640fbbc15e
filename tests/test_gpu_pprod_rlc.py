"""-m gpu: randomised pairing-product batches (blsmi 0.17).  The verdicts of blsmi_pairing_product_batch_rlc[_jac|_dev|_jac_dev] against the
oracle's per-item FinalExponentiation(MillerLoop(item)) on the corpus of tests/pprod_rlc_corpus.py (a table of 9 G2 entries: two shared by
most items, private ones, one used by two items, one unreferenced, one all-zero, one with the bytes of another; items of 0 to 5 pairs), and
`combined` saying which path gave them.  tests/test_pprod_rlc_cpu.py confirms the equation on the oracle alone."""
import numpy as np
import pytest

from gpu_common import P, g1_to_jac, g2_to_jac, jac1, jac2
from pprod_rlc_corpus import X, Y, Corpus, g1, g2, neg1

pytestmark = pytest.mark.gpu

BAD1, BAD2 = (2,), (7, 21)                                                      # a Groth16-shaped item; an item of the two-item entry and a two-pair item


def _defaults(engine):
    engine.set_latency_threshold(8192); engine.set_quad_threshold(16384); engine.set_row_threshold(*engine.ROW_DEFAULT)
    engine.set_option("segsum_chunk", 0)


@pytest.fixture(scope="module")
def eng():
    from bls_amd import engine
    engine.init(0)
    yield engine
    _defaults(engine)


@pytest.fixture(scope="module")
def corpora():
    """the corpus where every item holds, with one failing item, with two; the oracle's verdicts of each (computed once)"""
    base = Corpus()
    v0 = base.verdicts()
    assert all(v0) and 90 <= base.np <= 110
    out = {(): (base, v0)}
    for bad in (BAD1, BAD2):
        c = Corpus(bad)
        v = c.verdicts({j: v0[j] for j in range(len(v0)) if j not in bad})
        assert v == [0 if j in bad else 1 for j in range(len(v0))]
        out[bad] = (c, v)
    return out


def _host(eng, c, scalars=None, flags=True):
    return eng.pairing_product_batch_rlc(b"".join(c.g1s), b"".join(c.tab), c.q_idx, c.seg_off, c.flags if flags else None, scalars)


def _pinned(m):
    return [(0x9e3779b97f4a7c15 * (j + 1)) % (1 << 64) | 1 for j in range(m)]


def test_all_items_hold(eng, corpora):
    _defaults(eng)
    c, v = corpora[()]
    for scalars in (None, _pinned(len(v))):
        one, comb = _host(eng, c, scalars)
        assert one.tolist() == v == [1] * len(v)
        assert comb == 1                         # the cancelling group, the flagged P and the all-zero entry did not force the per-item path
    # is_one is what the 0.10 call gives on the expanded table
    _, want = eng.pairing_product_batch(b"".join(c.g1s), b"".join(c.tab[e] for e in c.q_idx), c.seg_off, c.flags)
    assert want.tolist() == v


@pytest.mark.parametrize("bad", [BAD1, BAD2])
def test_failing_items_among_them(eng, corpora, bad):
    _defaults(eng)
    c, v = corpora[bad]
    for scalars in (None, _pinned(len(v))):
        one, comb = _host(eng, c, scalars)
        assert comb == 0
        assert one.tolist() == v
    _, want = eng.pairing_product_batch(b"".join(c.g1s), b"".join(c.tab[e] for e in c.q_idx), c.seg_off, c.flags)
    assert want.tolist() == v


def test_the_cancelling_pair(eng):
    """two failing items with values v and 1 / v: the weights reach the equation per item"""
    _defaults(eng)
    p = g1(99)
    a, tab = p + neg1(p), g2(X)
    for q_idx, t in (([0, 0], tab), (None, tab + tab)):
        one, comb = eng.pairing_product_batch_rlc(a, t, q_idx, [0, 1, 2], scalars=[5, 5])
        assert (one.tolist(), comb) == ([1, 1], 1), q_idx                      # one group whose sum is infinity / two Miller values that cancel
        for scalars in ([5, 6], None):
            one, comb = eng.pairing_product_batch_rlc(a, t, q_idx, [0, 1, 2], scalars=scalars)
            assert (one.tolist(), comb) == ([0, 0], 0), (q_idx, scalars)


def _private_tables(n_items, bad=()):
    """n_items two-pair items, every pair with a table entry of its own (copies of Q_A and Q_B: equal bytes are not merged)"""
    xs = P.XORShift(321)
    qa, qb = g2(X), g2(Y)
    g1s, tab = [], []
    for j in range(n_items):
        s = P.rand_fr(xs)
        g1s += [g1(s * Y + (1 if j in bad else 0)), neg1(g1(s * X))]
        tab += [qa, qb]
    return g1s, tab, [2 * j for j in range(n_items + 1)]


def test_q_idx_null_all_singletons(eng):
    _defaults(eng)
    for bad in ((), (0, 34), (17,)):
        g1s, tab, off = _private_tables(35, bad)                                # 70 pairs, nq == np
        want = [0 if j in bad else 1 for j in range(35)]
        assert eng.pairing_product_batch(b"".join(g1s), b"".join(tab), off)[1].tolist() == want
        one, comb = eng.pairing_product_batch_rlc(b"".join(g1s), b"".join(tab), None, off)
        assert one.tolist() == want and comb == (0 if bad else 1), bad


def test_a_single_shared_entry(eng):
    _defaults(eng)
    tab = g2(Y)
    for bad in (False, True):                                                   # d' = 1: items (aP, Q), (-aP, Q)
        g1s = []
        for j in range(3):
            g1s += [g1(100 + j), neg1(g1(100 + j + (1 if bad and j == 1 else 0)))]
        one, comb = eng.pairing_product_batch_rlc(b"".join(g1s), tab, [0] * 6, [0, 2, 4, 6])
        assert (one.tolist(), comb) == (([1, 0, 1], 0) if bad else ([1, 1, 1], 1))
    # a table entry nobody refers to is never touched: garbage there changes nothing
    one, comb = eng.pairing_product_batch_rlc(b"".join(g1s[:2]), b"\xff" * 192 + tab, [1, 1], [0, 2])
    assert (one.tolist(), comb) == ([1], 1)


def test_empty_batches(eng):
    _defaults(eng)
    one, comb = eng.pairing_product_batch_rlc(b"", g2(X), [], [0, 0, 0, 0])
    assert (one.tolist(), comb) == ([1, 1, 1], 1)
    one, comb = eng.pairing_product_batch_rlc(b"", b"", None, [0, 0, 0, 0])
    assert (one.tolist(), comb) == ([1, 1, 1], 1)
    one, comb = eng.pairing_product_batch_rlc(b"", b"", None, [0])
    assert (one.tolist(), comb) == ([], 0)


def _t(b):
    import torch
    a = np.frombuffer(bytes(b), dtype=np.uint8).copy() if not isinstance(b, np.ndarray) else np.ascontiguousarray(b).view(np.uint8).reshape(-1).copy()
    if a.size == 0:
        a = np.zeros(8, dtype=np.uint8)
    return torch.from_numpy(a).to(torch.device("cuda", 0))


def _jac_corpus(c, seed):
    xs = P.XORShift(seed)
    j1 = [g1_to_jac(p, 0) if f else jac1(xs, p) for p, f in zip(c.g1s, c.flags)]
    j2 = [g2_to_jac(None) if q == bytes(192) else jac2(xs, q) for q in c.tab]
    return b"".join(j1), b"".join(j2)


@pytest.mark.parametrize("bad", [(), BAD1])
def test_every_form(eng, corpora, bad):
    import torch
    _defaults(eng)
    c, v = corpora[bad]
    m, nq = len(v), len(c.tab)
    scalars = _pinned(m)
    held = 0 if bad else 1
    j1, j2 = _jac_corpus(c, 5)
    one, comb = eng.pairing_product_batch_rlc_jac(j1, j2, c.q_idx, c.seg_off, scalars)
    assert one.tolist() == v and comb == held
    d_off, d_q, d_fl = _t(c.seg_off), _t(c.q_idx), _t(c.flags)
    st = torch.cuda.Stream(device=d_off.device)
    for jac in (False, True):
        d1, d2 = (_t(j1), _t(j2)) if jac else (_t(b"".join(c.g1s)), _t(b"".join(c.tab)))
        keep = [t.clone() for t in (d1, d2, d_off, d_q, d_fl)]
        for stream, sc in ((0, scalars), (st.cuda_stream, None)):
            d_one = torch.full((m,), 7, dtype=torch.uint8, device=d1.device)
            if jac:
                comb = eng.pairing_product_batch_rlc_jac_dev(d1.data_ptr(), d2.data_ptr(), nq, d_q.data_ptr(), c.np, d_off.data_ptr(), m, d_one.data_ptr(), scalars=sc, stream=stream)
            else:
                comb = eng.pairing_product_batch_rlc_dev(d1.data_ptr(), d2.data_ptr(), nq, d_q.data_ptr(), c.np, d_off.data_ptr(), m, d_one.data_ptr(),
                                                         d_inf_flags=d_fl.data_ptr(), scalars=sc, stream=stream)
            assert d_one.cpu().numpy().tolist() == v and comb == held, (jac, stream)
        for t, k in zip((d1, d2, d_off, d_q, d_fl), keep):
            assert torch.equal(t, k), "the caller's device buffers are byte-identical afterwards"
    # every group through the segmented sum (the by-pass's other side): the same verdicts
    d1, d2 = _t(b"".join(c.g1s)), _t(b"".join(c.tab))
    d_one = torch.full((m,), 7, dtype=torch.uint8, device=d1.device)
    comb = eng.pairing_product_batch_rlc_dev(d1.data_ptr(), d2.data_ptr(), nq, d_q.data_ptr(), c.np, d_off.data_ptr(), m, d_one.data_ptr(), d_inf_flags=d_fl.data_ptr(),
                                             scalars=scalars, nosplit=True)
    assert d_one.cpu().numpy().tolist() == v and comb == held


def _profiled(fn):
    import bench
    from bls_amd import _native
    lib = _native.load()
    bench.read_profile(lib)
    lib.blsmi_set_profiling(1)
    try:
        out = fn()
    finally:
        lib.blsmi_set_profiling(0)
    return out, bench.read_profile(lib)


def test_layouts_and_chunks(eng, corpora):
    """the d' = 40 Miller loops of 20 private-table items in the wave, row, quad and pair layouts, and the corpus's weighted sums under chunk
    sizes 2, 3 and 1 024: the verdicts do not move"""
    g1s, tab, off = _private_tables(20, (3,))
    want = [0 if j == 3 else 1 for j in range(20)]
    g1h, tabh, _ = _private_tables(20)
    combos = [
        (lambda: (eng.set_row_threshold(1, 1 << 20),), "k_miller1h_row"),
        (lambda: (eng.set_row_threshold(0, 0), eng.set_latency_threshold(0), eng.set_quad_threshold(1 << 20)), "k_miller1h_quad"),
        (lambda: (eng.set_row_threshold(0, 0), eng.set_latency_threshold(0), eng.set_quad_threshold(0)), "k_miller1h_pair"),
        (lambda: (eng.set_row_threshold(0, 0), eng.set_latency_threshold(8192), eng.set_quad_threshold(0)), "k_lat:miller1raw"),
    ]
    try:
        for setup, miller in combos:
            _defaults(eng)
            setup()
            (one, comb), prof = _profiled(lambda: eng.pairing_product_batch_rlc(b"".join(g1h), b"".join(tabh), None, off))
            assert miller in prof and "k_pprod_rlc_weights" in prof and "k_g1_mul_u64_idx" in prof and "k_fq12_seg_prod_row" in prof, (miller, sorted(prof))
            assert (one.tolist(), comb) == ([1] * 20, 1), miller
            one, comb = eng.pairing_product_batch_rlc(b"".join(g1s), b"".join(tab), None, off)
            assert (one.tolist(), comb) == (want, 0), miller
            for bad in ((), BAD2):
                c, v = corpora[bad]
                one, comb = _host(eng, c, _pinned(len(v)))
                assert (one.tolist(), comb) == (v, 0 if bad else 1), (miller, bad)
        _defaults(eng)
        for K in (2, 3, 1024):
            eng.set_option("segsum_chunk", K)
            for bad in ((), BAD1):
                c, v = corpora[bad]
                (one, comb), prof = _profiled(lambda: _host(eng, c, _pinned(len(v))))
                assert "k_g1_segsum_chunk_u64" in prof, sorted(prof)
                assert (one.tolist(), comb) == (v, 0 if bad else 1), (K, bad)
    finally:
        _defaults(eng)


def test_dev_form_refuses_a_bad_index(eng, corpora):
    import torch
    _defaults(eng)
    c, v = corpora[()]
    m, nq = len(v), len(c.tab)
    q = c.q_idx.copy(); q[5] = nq
    d1, d2, d_off, d_q = _t(b"".join(c.g1s)), _t(b"".join(c.tab)), _t(c.seg_off), _t(q)
    d_one = torch.full((m,), 7, dtype=torch.uint8, device=d1.device)
    with pytest.raises(eng.BlsmiError, match="bad argument"):
        eng.pairing_product_batch_rlc_dev(d1.data_ptr(), d2.data_ptr(), nq, d_q.data_ptr(), c.np, d_off.data_ptr(), m, d_one.data_ptr())
    assert d_one.cpu().numpy().tolist() == [7] * m, "nothing is written"
    bad_off = c.seg_off.copy(); bad_off[-1] -= 1
    d_good_q, d_bad_off, d_fl = _t(c.q_idx), _t(bad_off), _t(c.flags)
    with pytest.raises(eng.BlsmiError, match="bad argument"):
        eng.pairing_product_batch_rlc_dev(d1.data_ptr(), d2.data_ptr(), nq, d_good_q.data_ptr(), c.np, d_bad_off.data_ptr(), m, d_one.data_ptr())
    assert d_one.cpu().numpy().tolist() == [7] * m
    # and the library still serves a good call afterwards
    comb = eng.pairing_product_batch_rlc_dev(d1.data_ptr(), d2.data_ptr(), nq, d_good_q.data_ptr(), c.np, d_off.data_ptr(), m, d_one.data_ptr(), d_inf_flags=d_fl.data_ptr())
    assert d_one.cpu().numpy().tolist() == v and comb == 1
