"""-m gpu: randomised pairing-product batches that find the bad items by blocks (blsmi 0.18).  The verdicts of
blsmi_pairing_product_batch_rlc_locate[_jac|_dev|_jac_dev] against the oracle's per-item FinalExponentiation(MillerLoop(item)) and the 0.10
call on the corpus of tests/pprod_rlc_corpus.py, `combined` saying whether the one equation held and `rechecked` how many items the
per-item path saw: the summed sizes of the blocks with a failing item.  tests/test_pprod_rlc_locate_cpu.py confirms the block equations on
the oracle alone."""
import pytest

from pprod_rlc_corpus import DUP, UNREF, X, Y, Corpus, g1, g2, neg1
from pprod_rlc_locate_common import BAD1, BAD2, BLOCKS, rechecked_of
from test_gpu_pprod_rlc import _defaults, _jac_corpus, _pinned, _private_tables, _profiled, _t

pytestmark = pytest.mark.gpu

TAIL = (32,)                                                                    # the single item of the tail block at block 8
NEIGHBOURS = (2, 7, 10)                                                         # beside the empty items 1 and 11, the flagged-P item 3, the cancelling item 6, the all-zero-entry item 9
DUPBAD = (14,)                                                                  # the item of the entry with Q_A's bytes once more


@pytest.fixture(scope="module")
def eng():
    from bls_amd import engine
    engine.init(0)
    yield engine
    _defaults(engine)


@pytest.fixture(scope="module")
def corpora(eng):
    """the corpus where every item holds and with failing items; the oracle's verdicts of each (computed once), confirmed by the 0.10 call"""
    _defaults(eng)
    base = Corpus()
    v0 = base.verdicts()
    assert all(v0) and len(v0) == 33 and 90 <= base.np <= 110
    assert base.items[1] == [] and base.items[11] == [] and len(base.items[32]) == 2
    out = {(): (base, v0)}
    for bad in (BAD1, BAD2, TAIL, NEIGHBOURS, DUPBAD):
        c = Corpus(bad)
        v = c.verdicts({j: v0[j] for j in range(len(v0)) if j not in bad})
        assert v == [0 if j in bad else 1 for j in range(len(v0))]
        out[bad] = (c, v)
    for bad, (c, v) in out.items():
        _, want = eng.pairing_product_batch(b"".join(c.g1s), b"".join(c.tab[e] for e in c.q_idx), c.seg_off, c.flags)
        assert want.tolist() == v, bad
    return out


def _host(eng, c, block, scalars=None, tab=None):
    return eng.pairing_product_batch_rlc_locate(b"".join(c.g1s), b"".join(tab or c.tab), c.q_idx, c.seg_off, c.flags, scalars, block)


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("bad", [(), BAD1, BAD2])
def test_verdicts_combined_and_rechecked(eng, corpora, bad, block):
    _defaults(eng)
    c, v = corpora[bad]
    m = len(v)
    want_re = rechecked_of(m, block, bad)
    if block == 8:
        assert want_re == {(): 0, BAD1: 8, BAD2: 16}[bad]
    elif block == 1:
        assert want_re == len(bad)
    else:
        assert want_re == (33 if bad else 0)
    for scalars in (None, _pinned(m)):
        one, comb, nre = _host(eng, c, block, scalars)
        assert one.tolist() == v, (bad, block)
        assert comb == (0 if bad else 1)     # all valid: the cancelling cell, the flagged P and the all-zero entry did not force the per-item path
        assert nre == want_re, (bad, block)


def test_a_bad_item_alone_in_the_tail_block(eng, corpora):
    _defaults(eng)
    c, v = corpora[TAIL]
    one, comb, nre = _host(eng, c, 8, _pinned(len(v)))
    assert (one.tolist(), comb, nre) == (v, 0, 1)


def test_edges_of_the_route_at_block_one(eng, corpora):
    """block = 1: the cancelling item, the flagged-P item, the all-zero-entry item and the two empty items are each a block of their own
    (a cell whose sum is infinity, a cell of nothing, a dropped cell, no cell at all) beside blocks whose Q_A cells are finite"""
    _defaults(eng)
    c, v = corpora[()]
    for scalars in (None, _pinned(len(v))):
        one, comb, nre = _host(eng, c, 1, scalars)
        assert (one.tolist(), comb, nre) == (v, 1, 0)
    c, v = corpora[NEIGHBOURS]
    for scalars in (None, _pinned(len(v))):
        one, comb, nre = _host(eng, c, 1, scalars)
        assert (one.tolist(), comb, nre) == (v, 0, len(NEIGHBOURS)), "only the bad neighbours are rechecked"
    # the entry with Q_A's bytes once more is a table entry of its own: its item fails alone
    c, v = corpora[DUPBAD]
    one, comb, nre = _host(eng, c, 1, _pinned(len(v)))
    assert (one.tolist(), comb, nre) == (v, 0, 1)
    assert c.tab[DUP] == c.tab[0]
    # a table entry nobody refers to is never touched: garbage there changes nothing
    for bad in ((), BAD2):
        c, v = corpora[bad]
        tab = list(c.tab); tab[UNREF] = b"\xff" * 192
        one, comb, nre = _host(eng, c, 1, _pinned(len(v)), tab)
        assert (one.tolist(), comb, nre) == (v, 0 if bad else 1, len(bad))


def test_the_cancelling_pair(eng):
    """two failing items with values v and 1 / v under pinned scalars: equal scalars pass -- in different blocks too, because the total
    holds -- and scalars (5, 6) fail both blocks"""
    _defaults(eng)
    p = g1(99)
    a, tab = p + neg1(p), g2(X)
    for q_idx, t in (([0, 0], tab), (None, tab + tab)):
        for block in (1, 2):
            one, comb, nre = eng.pairing_product_batch_rlc_locate(a, t, q_idx, [0, 1, 2], scalars=[5, 5], block=block)
            assert (one.tolist(), comb, nre) == ([1, 1], 1, 0), (q_idx, block)
            for scalars in ([5, 6], None):
                one, comb, nre = eng.pairing_product_batch_rlc_locate(a, t, q_idx, [0, 1, 2], scalars=scalars, block=block)
                assert (one.tolist(), comb, nre) == ([0, 0], 0, 2), (q_idx, block, scalars)


def test_q_idx_null_all_one_pair_cells(eng):
    _defaults(eng)
    for bad in ((), (17,), (0, 34)):
        g1s, tab, off = _private_tables(35, bad)                                # 70 pairs, nq == np
        want = [0 if j in bad else 1 for j in range(35)]
        assert eng.pairing_product_batch(b"".join(g1s), b"".join(tab), off)[1].tolist() == want
        for block in (0, 1, 8):
            one, comb, nre = eng.pairing_product_batch_rlc_locate(b"".join(g1s), b"".join(tab), None, off, block=block)
            assert (one.tolist(), comb, nre) == (want, 0 if bad else 1, rechecked_of(35, block, bad)), (bad, block)


def test_a_single_shared_entry(eng):
    _defaults(eng)
    tab = g2(Y)
    for block in (1, 2, 3):
        for bad in (False, True):                                               # d' = 1: items (aP, Q), (-aP, Q)
            g1s = []
            for j in range(3):
                g1s += [g1(100 + j), neg1(g1(100 + j + (1 if bad and j == 1 else 0)))]
            one, comb, nre = eng.pairing_product_batch_rlc_locate(b"".join(g1s), tab, [0] * 6, [0, 2, 4, 6], block=block)
            assert (one.tolist(), comb, nre) == (([1, 0, 1], 0, rechecked_of(3, block, (1,))) if bad else ([1, 1, 1], 1, 0)), (block, bad)


def test_empty_batches(eng):
    _defaults(eng)
    for block in (0, 1, 2):
        one, comb, nre = eng.pairing_product_batch_rlc_locate(b"", g2(X), [], [0, 0, 0, 0], block=block)
        assert (one.tolist(), comb, nre) == ([1, 1, 1], 1, 0)
        one, comb, nre = eng.pairing_product_batch_rlc_locate(b"", b"", None, [0, 0, 0, 0], block=block)
        assert (one.tolist(), comb, nre) == ([1, 1, 1], 1, 0)
        one, comb, nre = eng.pairing_product_batch_rlc_locate(b"", b"", None, [0], block=block)
        assert (one.tolist(), comb, nre) == ([], 0, 0)


@pytest.mark.parametrize("bad", [(), BAD2])
def test_every_form(eng, corpora, bad):
    import torch
    _defaults(eng)
    c, v = corpora[bad]
    m, nq = len(v), len(c.tab)
    scalars = _pinned(m)
    held, want_re = (0 if bad else 1), rechecked_of(m, 8, bad)
    j1, j2 = _jac_corpus(c, 5)
    one, comb, nre = eng.pairing_product_batch_rlc_locate_jac(j1, j2, c.q_idx, c.seg_off, scalars, 8)
    assert (one.tolist(), comb, nre) == (v, held, want_re)
    d_off, d_q, d_fl = _t(c.seg_off), _t(c.q_idx), _t(c.flags)
    st = torch.cuda.Stream(device=d_off.device)
    for jac in (False, True):
        d1, d2 = (_t(j1), _t(j2)) if jac else (_t(b"".join(c.g1s)), _t(b"".join(c.tab)))
        keep = [t.clone() for t in (d1, d2, d_off, d_q, d_fl)]
        for stream, sc in ((0, scalars), (st.cuda_stream, None)):
            d_one = torch.full((m,), 7, dtype=torch.uint8, device=d1.device)
            if jac:
                got = eng.pairing_product_batch_rlc_locate_jac_dev(d1.data_ptr(), d2.data_ptr(), nq, d_q.data_ptr(), c.np, d_off.data_ptr(), m, d_one.data_ptr(), scalars=sc,
                                                                   block=8, stream=stream)
            else:
                got = eng.pairing_product_batch_rlc_locate_dev(d1.data_ptr(), d2.data_ptr(), nq, d_q.data_ptr(), c.np, d_off.data_ptr(), m, d_one.data_ptr(),
                                                               d_inf_flags=d_fl.data_ptr(), scalars=sc, block=8, stream=stream)
            assert d_one.cpu().numpy().tolist() == v and got == (held, want_re), (jac, stream)
        for t, k in zip((d1, d2, d_off, d_q, d_fl), keep):
            assert torch.equal(t, k), "the caller's device buffers are byte-identical afterwards"


def test_dev_form_over_g1_records_that_are_only_word_aligned(eng, corpora):
    """the caller's G1 records 4 bytes into a buffer: the recheck's gather then moves words, not 16-byte pieces"""
    import torch
    _defaults(eng)
    c, v = corpora[BAD2]
    m, nq = len(v), len(c.tab)
    raw = b"".join(c.g1s)
    buf = _t(b"\xa5" * 4 + raw + b"\xa5" * 12)
    d1 = buf[4:4 + len(raw)]
    assert d1.data_ptr() % 16 == 4
    d2, d_off, d_q, d_fl = _t(b"".join(c.tab)), _t(c.seg_off), _t(c.q_idx), _t(c.flags)
    keep = buf.clone()
    d_one = torch.full((m,), 7, dtype=torch.uint8, device=buf.device)
    got = eng.pairing_product_batch_rlc_locate_dev(d1.data_ptr(), d2.data_ptr(), nq, d_q.data_ptr(), c.np, d_off.data_ptr(), m, d_one.data_ptr(),
                                                   d_inf_flags=d_fl.data_ptr(), scalars=_pinned(m), block=8)
    assert d_one.cpu().numpy().tolist() == v and got == (0, 16)
    assert torch.equal(buf, keep)


def test_dev_forms_refuse_a_bad_index_or_offset(eng, corpora):
    import torch
    _defaults(eng)
    c, v = corpora[()]
    m, nq = len(v), len(c.tab)
    q = c.q_idx.copy(); q[5] = nq
    bad_off = c.seg_off.copy(); bad_off[-1] -= 1
    j1, j2 = _jac_corpus(c, 5)
    d_off, d_q, d_good_q, d_bad_off, d_fl = _t(c.seg_off), _t(q), _t(c.q_idx), _t(bad_off), _t(c.flags)
    for jac in (False, True):
        d1, d2 = (_t(j1), _t(j2)) if jac else (_t(b"".join(c.g1s)), _t(b"".join(c.tab)))
        f = eng.pairing_product_batch_rlc_locate_jac_dev if jac else eng.pairing_product_batch_rlc_locate_dev
        d_one = torch.full((m,), 7, dtype=torch.uint8, device=d1.device)
        with pytest.raises(eng.BlsmiError, match="bad argument"):
            f(d1.data_ptr(), d2.data_ptr(), nq, d_q.data_ptr(), c.np, d_off.data_ptr(), m, d_one.data_ptr(), block=8)
        assert d_one.cpu().numpy().tolist() == [7] * m, "nothing is written"
        with pytest.raises(eng.BlsmiError, match="bad argument"):
            f(d1.data_ptr(), d2.data_ptr(), nq, d_good_q.data_ptr(), c.np, d_bad_off.data_ptr(), m, d_one.data_ptr(), block=8)
        assert d_one.cpu().numpy().tolist() == [7] * m
        # and the library still serves a good call afterwards
        kw = {} if jac else {"d_inf_flags": d_fl.data_ptr()}
        got = f(d1.data_ptr(), d2.data_ptr(), nq, d_good_q.data_ptr(), c.np, d_off.data_ptr(), m, d_one.data_ptr(), block=8, **kw)
        assert d_one.cpu().numpy().tolist() == v and got == (1, 0)


def test_layouts_and_chunks(eng, corpora):
    """the C = 40 Miller loops of 20 private-table items in the wave, row, quad and pair layouts (thresholds forced as
    tests/test_gpu_pprod_rlc.py forces them; the block values' final exponentiations follow them too), and the corpus's weighted sums under
    chunk sizes 2, 3 and 1 024: the verdicts and `rechecked` do not move"""
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
            (one, comb, nre), prof = _profiled(lambda: eng.pairing_product_batch_rlc_locate(b"".join(g1h), b"".join(tabh), None, off, block=4))
            for name in (miller, "k_pprod_rlc_weights", "k_g1_mul_u64_idx", "k_pprod_cell_route", "k_fq12_seg_prod_row"):
                assert name in prof, (miller, name, sorted(prof))
            assert (one.tolist(), comb, nre) == ([1] * 20, 1, 0), miller
            (one, comb, nre), prof = _profiled(lambda: eng.pairing_product_batch_rlc_locate(b"".join(g1s), b"".join(tab), None, off, block=4))
            assert (one.tolist(), comb, nre) == (want, 0, 4), miller
            for name in (miller, "k_pprod_cell_route", "k_gather_records16", "k_scatter_bytes"):
                assert name in prof, (miller, name, sorted(prof))
            for bad in ((), BAD2):
                c, v = corpora[bad]
                for block in (1, 8):
                    one, comb, nre = _host(eng, c, block, _pinned(len(v)))
                    assert (one.tolist(), comb, nre) == (v, 0 if bad else 1, rechecked_of(len(v), block, bad)), (miller, bad, block)
        _defaults(eng)
        for K in (2, 3, 1024):
            eng.set_option("segsum_chunk", K)
            for bad in ((), BAD1):
                c, v = corpora[bad]
                (one, comb, nre), prof = _profiled(lambda: _host(eng, c, 8, _pinned(len(v))))
                assert "k_g1_segsum_chunk_u64" in prof and "k_pprod_cell_route" in prof, sorted(prof)
                assert (one.tolist(), comb, nre) == (v, 0 if bad else 1, rechecked_of(len(v), 8, bad)), (K, bad)
    finally:
        _defaults(eng)
