"""-m gpu: the Miller-loop variants that tests/test_gpu_launch_table.py does not name.  The loops over the bits of |x| are written once for the
single-lane, lane-pair and lane-quad layouts (pairing_body.inc: x_bit_walk), every kernel there one set of actions handed to the walker; the
lane-row loops are written out (row_body.inc).  The launch-table tests run k_miller1h_{row,quad,pair}, k_miller1m_row and k_miller2_{quad,pair}
with and without the generator's table.  Here, with the layout forced by the run-time setters and the kernel's name read from blsmi_last_profile:

  k_miller1_pair          one pair, the reference's exact steps (MillerLoop)
  k_miller1_prep_pair     one pair, its lines read from the key's table
  k_miller2_prep_pair     two pairs, both from tables
  k_miller1x2_prep_pair   an aggregate's loops over tables, two tuples a lane pair
  k_miller1x2_pair/_quad  an aggregate's loops, two tuples a lane pair / quad
  k_miller2_row           two pairs in the row layout, with the generator's table (g2pubs) and without (g1pubs)

Counts: 1; one more than a workgroup holds (33 tuples for the pair layout's one-pair kernels, 5 for the row layout; for the kernels that take two
tuples at a time 65 for the pair and 33 for the quad layout); and for those kernels 2 and 3 -- 3 puts a full pair and the odd tuple out, which
runs a one-pair loop beside the others' two-pair loop, in one wave.  Values and verdicts are the oracle's."""
import ctypes

import numpy as np
import pytest

from gpu_common import P, RC, rand_g1, rand_g2, sk_bytes

pytestmark = pytest.mark.gpu
NS = 66                                                                    # 65 signers and one key that signs nothing here


@pytest.fixture(scope="module")
def eng():
    from bls_amd import engine
    engine.init(0)
    yield engine


@pytest.fixture
def layout_of(eng):
    def force(layout):
        if layout == "row":
            eng.set_row_threshold(1, 8192)
        else:
            eng.set_row_threshold(0, 0); eng.set_latency_threshold(0)
            if layout == "pair":
                eng.set_quad_threshold(0)
    yield force
    eng.set_latency_threshold(8192); eng.set_quad_threshold(16384); eng.set_row_threshold(*eng.ROW_DEFAULT)
    eng.set_option("row_side", 1)


def names_of(eng, call):
    """call() with profiling on -> (its result, the names of blsmi_last_profile in order)"""
    lib = eng._lib()
    buf = ctypes.create_string_buffer(1 << 14)
    lib.blsmi_set_profiling(1); lib.blsmi_last_profile(buf, ctypes.c_size_t(len(buf)))
    try:
        out = call()
    finally:
        lib.blsmi_set_profiling(0)
    lib.blsmi_last_profile(buf, ctypes.c_size_t(len(buf)))
    return out, [item.split("=")[0] for item in buf.value.decode().split(";") if item]


def _dev(x):
    import torch
    a = np.frombuffer(x, dtype=np.uint8).copy() if isinstance(x, (bytes, bytearray)) else np.ascontiguousarray(x)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(torch.device("cuda", 0))


def _msgs_dev(msgs):
    off = np.zeros(len(msgs) + 1, dtype=np.uint64); off[1:] = np.cumsum([len(m) for m in msgs])
    return _dev(b"".join(msgs)), _dev(off)


def _tables(eng, keys):
    import torch
    tab = torch.empty(len(keys) * eng.G2_PREPARED_BYTES, dtype=torch.uint8, device=torch.device("cuda", 0))
    eng.g2_prepare_batch_dev(_dev(b"".join(keys)).data_ptr(), len(keys), tab.data_ptr())
    return tab


@pytest.fixture(scope="module")
def points():
    xs = P.XORShift(1401)
    n = 33
    g1 = [rand_g1(xs) for _ in range(n)]; g2 = [rand_g2(xs) for _ in range(n)]
    return g1, g2, np.stack([RC.miller_loop(a, b, 1) for a, b in zip(g1, g2)]), RC.pairing_batch(b"".join(g1), b"".join(g2), n)


@pytest.fixture(scope="module")
def signed():
    """NS keys of both packages, one message each, and the oracle's signatures"""
    xs = P.XORShift(1402)
    sks = [sk_bytes(xs) for _ in range(NS)]
    msgs = [b"miller variant %d" % i + bytes(i % 3) for i in range(NS)]
    return {name: (msgs, [o.priv_to_pub(k) for k in sks], [o.sign(m, k) for m, k in zip(msgs, sks)])
            for name, o in (("g2pubs", RC.g2pubs), ("g1pubs", RC.g1pubs))}


@pytest.mark.parametrize("n", [1, 33])
def test_exact_one_pair_loop(eng, layout_of, points, n):
    g1, g2, ml, _ = points
    layout_of("pair")
    got, names = names_of(eng, lambda: eng.miller_loop_batch(b"".join(g1[:n]), b"".join(g2[:n]), n))
    assert "k_miller1_pair" in names, names
    assert np.array_equal(got, ml[:n])


@pytest.mark.parametrize("n", [1, 33])
def test_one_pair_loop_over_a_prepared_key(eng, layout_of, points, n):
    import torch
    g1, g2, _, want = points
    layout_of("pair")
    tab = _tables(eng, g2[:n])
    d_g1 = _dev(b"".join(g1[:n]))
    out = torch.empty(n * 72, dtype=torch.int64, device=torch.device("cuda", 0))
    _, names = names_of(eng, lambda: eng.pairing_batch_prepared_dev(d_g1.data_ptr(), tab.data_ptr(), 0, out.data_ptr(), n))
    assert "k_miller1_prep_pair" in names, names
    assert np.array_equal(out.cpu().numpy().view(np.uint64).reshape(n, 72), want[:n])


@pytest.mark.parametrize("n", [1, 33])
def test_two_pair_loop_over_both_tables(eng, layout_of, signed, n):
    """g2pubs Verify over prepared keys: the last signature is another tuple's"""
    import torch
    msgs, pks, sigs = signed["g2pubs"]
    layout_of("pair")
    tab = _tables(eng, pks[:n])
    wrong = sigs[:n - 1] + [sigs[n]]
    expect = [True] * (n - 1) + [False]
    assert RC.g2pubs.verify(msgs[n - 1], pks[n - 1], wrong[n - 1]) is False and RC.g2pubs.verify(msgs[0], pks[0], sigs[0]) is True
    d_m, d_o = _msgs_dev(msgs[:n])
    d_s = _dev(b"".join(wrong))
    ok = torch.zeros(n, dtype=torch.uint8, device=torch.device("cuda", 0))
    _, names = names_of(eng, lambda: eng.g2pubs_verify_batch_prepared_dev(d_m.data_ptr(), d_o.data_ptr(), tab.data_ptr(), 0, d_s.data_ptr(), 0, ok.data_ptr(), n))
    assert "k_miller2_prep_pair" in names, names
    assert ok.cpu().numpy().astype(bool).tolist() == expect


AGGREGATES = [("pair", "k_miller1x2_pair", n) for n in (1, 2, 3, 65)] + [("quad", "k_miller1x2_quad", n) for n in (1, 2, 3, 33)]


@pytest.mark.parametrize("layout,kernel,n", AGGREGATES, ids=["%s-%d" % (a[0], a[2]) for a in AGGREGATES])
@pytest.mark.parametrize("group", ["g2pubs", "g1pubs"])
def test_aggregate_loops_two_tuples_at_a_time(eng, layout_of, signed, group, layout, kernel, n):
    """valid; then the LAST key replaced -- the odd tuple out where n is odd -- and the first"""
    msgs, pks, sigs = signed[group]
    o = RC.g2pubs if group == "g2pubs" else RC.g1pubs
    fn, summ = (eng.g2pubs_verify_aggregate, eng.g1_sum) if group == "g2pubs" else (eng.g1pubs_verify_aggregate, eng.g2_sum)
    agg = summ(b"".join(sigs[:n]), n)
    layout_of(layout)
    ok, names = names_of(eng, lambda: fn(msgs[:n], b"".join(pks[:n]), agg))
    assert kernel in names, names
    assert ok is True and o.verify_aggregate(agg, pks[:n], msgs[:n]) is True
    for at in (n - 1, 0):
        wrong = list(pks[:n]); wrong[at] = pks[n]
        assert fn(msgs[:n], b"".join(wrong), agg) is False and o.verify_aggregate(agg, wrong, msgs[:n]) is False


@pytest.mark.parametrize("n", [1, 2, 3, 65])
def test_aggregate_loops_over_prepared_keys(eng, layout_of, signed, n):
    msgs, pks, sigs = signed["g2pubs"]
    agg = eng.g1_sum(b"".join(sigs[:n]), n)
    layout_of("pair")
    tab = _tables(eng, pks[:n + 1])
    d_m, d_o = _msgs_dev(msgs[:n])

    def call(idx):
        d_i = _dev(np.asarray(idx, dtype=np.uint32))
        return eng.g2pubs_verify_aggregate_prepared_dev(d_m.data_ptr(), d_o.data_ptr(), tab.data_ptr(), d_i.data_ptr(), agg, n)

    ok, names = names_of(eng, lambda: call(range(n)))
    assert "k_miller1x2_prep_pair" in names, names
    assert ok is True and RC.g2pubs.verify_aggregate(agg, pks[:n], msgs[:n]) is True
    for at in (n - 1, 0):
        idx = list(range(n)); idx[at] = n
        assert call(idx) is False and RC.g2pubs.verify_aggregate(agg, [pks[j] for j in idx], msgs[:n]) is False


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("group", ["g2pubs", "g1pubs"])
def test_two_pair_loop_in_the_row_layout(eng, layout_of, signed, group, n):
    """row_side = 0: one two-pair loop a tuple, g2pubs over the generator's table, g1pubs both points by their steps"""
    msgs, pks, sigs = signed[group]
    o = RC.g2pubs if group == "g2pubs" else RC.g1pubs
    fn = eng.g2pubs_verify_batch if group == "g2pubs" else eng.g1pubs_verify_batch
    wrong = sigs[:n - 1] + [sigs[n]]
    assert o.verify(msgs[n - 1], pks[n - 1], wrong[n - 1]) is False
    layout_of("row"); eng.set_option("row_side", 0)
    (ok, _), names = names_of(eng, lambda: fn(msgs[:n], b"".join(pks[:n]), b"".join(sigs[:n])))
    assert "k_miller2_row" in names, names
    assert list(ok) == [True] * n
    (ok, _), _ = names_of(eng, lambda: fn(msgs[:n], b"".join(pks[:n]), b"".join(wrong)))
    assert list(ok) == [True] * (n - 1) + [False]
