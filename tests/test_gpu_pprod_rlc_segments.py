"""-m gpu: what the randomised pairing-product batches launch (blsmi 0.17 blsmi_pairing_product_batch_rlc*, blsmi 0.18
blsmi_pairing_product_batch_rlc_locate*).  One call per case with profiling on; the ordered segment names of blsmi_last_profile (names only,
no times) against the lists below, which were recorded from the library as it stood before both forms were built from one set of host
stages (bls_amd/csrc/rlc_host.hpp): the stages launch what the two monoliths launched, in their order.  Every case also asserts the
verdicts, `combined` and `rechecked` that tests/test_gpu_pprod_rlc.py and tests/test_gpu_pprod_rlc_locate.py assert for the same input, so
that a wrong list cannot hide a wrong answer."""
import ctypes

import pytest

from pprod_rlc_corpus import Corpus
from pprod_rlc_locate_common import BAD2, rechecked_of
from test_gpu_pprod_rlc import _defaults, _jac_corpus, _pinned, _private_tables, _t

pytestmark = pytest.mark.gpu

BLOCK = 4

# The pieces of the lists.  A "(between)" runs from a closing mark to the next mark, or to the end of the context lease.
_WEIGHTS = ["k_pprod_rlc_weights", "(between)"]
_SEGSUM = ["k_g1_segsum_chunk_u64", "(between)"]                                # the multi-pair segments' weighted sum: one segment for its passes
_ONE_PAIR = ["k_g1_mul_u64_idx", "(between)"]                                   # the one-pair segments' ladders
_SUMS = _WEIGHTS + _SEGSUM + _ONE_PAIR
# the Miller loops (the wave layout at these sizes; k_pprod_skip before them is unmarked), the segmented product(s), the final
# exponentiation, the comparison with one -- of the one equation, and of blsmi_pairing_product_batch's own path
_PRODUCT = ["k_lat:miller1raw", "k_fq12_seg_prod_row", "k_lat:finalexp1", "k_fq12_is_one_m384", "(between)"]
_ROUTE = ["k_pprod_cell_route"]                                                 # 0.18: the cells into block order, right before their Miller loops
_BLOCKS = ["k_lat:finalexp1", "k_fq12_is_one_m384", "(between)"]                # 0.18, the total failed: which blocks fail
_RECHECK = ["k_gather_records16", "(between)"] + _PRODUCT + ["k_scatter_bytes", "(between)"]
_FROM_JAC = ["k_g1_jac_to_affine", "(between)", "k_g2_jac_to_affine", "(between)"]   # the in-memory forms: jac_to_wire_dev of the G1 points, of the gathered table entries
NAMES = {}


def _segments(eng, call):
    """call() with profiling on (as _profiled of tests/test_gpu_pprod_rlc.py turns it on) -> (its result, the names of the raw
    blsmi_last_profile string in order)"""
    lib = eng._lib()
    buf = ctypes.create_string_buffer(1 << 16)
    lib.blsmi_last_profile(buf, ctypes.c_size_t(len(buf)))                      # (read-and-clear)
    lib.blsmi_set_profiling(1)
    try:
        out = call()
    finally:
        lib.blsmi_set_profiling(0)
    lib.blsmi_last_profile(buf, ctypes.c_size_t(len(buf)))
    return out, [item.split("=")[0] for item in buf.value.decode().split(";") if item]


@pytest.fixture(scope="module")
def eng():
    from bls_amd import engine
    engine.init(0)
    yield engine
    _defaults(engine)


@pytest.fixture(scope="module")
def inputs():
    """the corpus where every item holds and with the two failing items of BAD2, the oracle's verdicts of each (computed once); 20 two-pair
    items over private table entries, item 3 failing"""
    base = Corpus()
    v0 = base.verdicts()
    assert all(v0) and len(v0) == 33 and 90 <= base.np <= 110
    bad = Corpus(BAD2)
    vb = bad.verdicts({j: v0[j] for j in range(len(v0)) if j not in BAD2})
    assert vb == [0 if j in BAD2 else 1 for j in range(len(v0))]
    return {"holds": (base, v0), "bad2": (bad, vb), "private": _private_tables(20, (3,))}


def _host(eng, c, block=None):
    m = len(c.seg_off) - 1
    if block is None:
        return eng.pairing_product_batch_rlc(b"".join(c.g1s), b"".join(c.tab), c.q_idx, c.seg_off, c.flags, _pinned(m)) + (None,)
    return eng.pairing_product_batch_rlc_locate(b"".join(c.g1s), b"".join(c.tab), c.q_idx, c.seg_off, c.flags, _pinned(m), block)


def _private(eng, tables, block=None):
    g1s, tab, off = tables
    if block is None:
        return eng.pairing_product_batch_rlc(b"".join(g1s), b"".join(tab), None, off, scalars=_pinned(20)) + (None,)
    return eng.pairing_product_batch_rlc_locate(b"".join(g1s), b"".join(tab), None, off, scalars=_pinned(20), block=block)


def _dev(eng, c, jac, block=None, nosplit=False):
    """the device-pointer forms; the uploads and the verdicts' way back lie outside the profiled call"""
    import torch
    m, nq = len(c.seg_off) - 1, len(c.tab)
    j1, j2 = _jac_corpus(c, 5)
    d1, d2 = (_t(j1), _t(j2)) if jac else (_t(b"".join(c.g1s)), _t(b"".join(c.tab)))
    d_off, d_q, d_fl = _t(c.seg_off), _t(c.q_idx), _t(c.flags)
    d_one = torch.full((m,), 7, dtype=torch.uint8, device=d1.device)
    args = (d1.data_ptr(), d2.data_ptr(), nq, d_q.data_ptr(), c.np, d_off.data_ptr(), m, d_one.data_ptr())
    kw = {"scalars": _pinned(m)}
    if not jac:
        kw["d_inf_flags"] = d_fl.data_ptr()
    if nosplit:
        kw["nosplit"] = True
    if block is not None:
        kw["block"] = block
    name = "pairing_product_batch_rlc" + ("" if block is None else "_locate") + ("_jac_dev" if jac else "_dev")

    def call():
        got = getattr(eng, name)(*args, **kw)
        return got if block is not None else (got, None)
    return call, lambda: d_one.cpu().numpy().tolist()


def _case(name, names):
    NAMES[name] = names
    return name


# the equation holds: the memset of the verdicts launches nothing.  It fails: blsmi_pairing_product_batch's own path over all 33 items
# (the table gather before it is unmarked)
@pytest.mark.parametrize("case", [
    _case("rlc_holds", _SUMS + _PRODUCT),
    _case("rlc_bad2", _SUMS + _PRODUCT + _PRODUCT),
])
def test_rlc_on_the_corpus(eng, inputs, case):
    _defaults(eng)
    c, v = inputs[case[len("rlc_"):]]
    (one, comb, _), names = _segments(eng, lambda: _host(eng, c))
    assert (one.tolist(), comb) == (v, 1 if case == "rlc_holds" else 0)
    assert names == NAMES[case]


# the cells' route right before their Miller loops; the blocks' products and the total's in one segment.  The total fails: the 9 blocks'
# final exponentiations and comparisons, the gathers of the two failing blocks' 8 items, the per-item path over them, the scatter
@pytest.mark.parametrize("case", [
    _case("locate_holds", _SUMS + _ROUTE + _PRODUCT),
    _case("locate_bad2", _SUMS + _ROUTE + _PRODUCT + _BLOCKS + _RECHECK),
])
def test_locate_on_the_corpus(eng, inputs, case):
    _defaults(eng)
    c, v = inputs[case[len("locate_"):]]
    (one, comb, nre), names = _segments(eng, lambda: _host(eng, c, BLOCK))
    want_re = rechecked_of(len(v), BLOCK, BAD2) if case == "locate_bad2" else 0
    assert want_re in (0, 8)
    assert (one.tolist(), comb, nre) == (v, 1 if case == "locate_holds" else 0, want_re)
    assert names == NAMES[case]


# q_idx == NULL: every pair a one-pair segment -- no segmented-sum pass at all
@pytest.mark.parametrize("case", [
    _case("private_rlc", _WEIGHTS + _ONE_PAIR + _PRODUCT + _PRODUCT),
    _case("private_locate", _WEIGHTS + _ONE_PAIR + _ROUTE + _PRODUCT + _BLOCKS + _RECHECK),
])
def test_private_tables_have_no_segmented_sum(eng, inputs, case):
    _defaults(eng)
    want = [0 if j == 3 else 1 for j in range(20)]
    block = BLOCK if case == "private_locate" else None
    (one, comb, nre), names = _segments(eng, lambda: _private(eng, inputs["private"], block))
    assert (one.tolist(), comb, nre) == (want, 0, 4 if block else None)
    assert not any("segsum" in n for n in names)
    assert names == NAMES[case]


# the device-pointer forms on the holding corpus: the table gather is unmarked; the in-memory forms convert the G1 points and the gathered
# table entries first (jac_to_wire_dev, once per group)
@pytest.mark.parametrize("case,jac,block,nosplit", [
    (_case("rlc_dev", _SUMS + _PRODUCT), False, None, False),
    (_case("rlc_jac_dev", _FROM_JAC + _SUMS + _PRODUCT), True, None, False),
    (_case("locate_dev", _SUMS + _ROUTE + _PRODUCT), False, BLOCK, False),
    (_case("locate_jac_dev", _FROM_JAC + _SUMS + _ROUTE + _PRODUCT), True, BLOCK, False),
    # every group through the segmented sum: no one-pair ladder
    (_case("nosplit", _WEIGHTS + _SEGSUM + _PRODUCT), False, None, True),
])
def test_dev_forms_on_the_holding_corpus(eng, inputs, case, jac, block, nosplit):
    _defaults(eng)
    c, v = inputs["holds"]
    call, verdicts = _dev(eng, c, jac, block, nosplit)
    (comb, nre), names = _segments(eng, call)
    assert (verdicts(), comb, nre) == (v, 1, None if block is None else 0)
    assert names == NAMES[case]
