"""-m gpu: pairing products (blsmi 0.10).  Item j = FinalExponentiation(MillerLoop(pairs of segment j)), bit for bit against the oracle
(infinite pairs dropped before the oracle call), against blsmi_pairing_batch for single-pair segments, and -- for segments of thousands
of pairs, where the oracle's Miller loops would take minutes -- against the oracle-side fq12_mul fold of the library's own pairing_batch
values (the final exponentiation is multiplicative).  Equations that hold are made as e(aP, Q) e(-P, aQ) = 1
(tests/test_pairing_product_cpu.py confirms the construction on the oracle alone)."""
import ctypes
import threading

import numpy as np
import pytest

from gpu_common import P, RC, g1_to_jac, g2_to_jac, jac1, jac2

pytestmark = pytest.mark.gpu


def _defaults(engine):
    engine.set_latency_threshold(8192); engine.set_quad_threshold(16384); engine.set_row_threshold(*engine.ROW_DEFAULT)
    engine.set_option("segsum_chunk", 0)


@pytest.fixture(scope="module")
def eng():
    from bls_amd import engine
    engine.init(0)
    yield engine
    _defaults(engine)


def _one():
    one = np.zeros(72, dtype=np.uint64)
    one[:6] = np.array(P.limbs64(P.to_mont(1)), dtype=np.uint64)
    return one


ONE = _one()


def _neg1(p):
    return p[:48] + ((P.Q - int.from_bytes(p[48:], "big")) % P.Q).to_bytes(48, "big")


def _scalars(seed, n):
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 0] &= 0x3f
    return s


def _points(eng, n, seed):
    """n random pairs: lists of 96-byte G1 and 192-byte G2 affine records (multiples of the generators, made on the device)"""
    a, _ = eng.g1_mul_generator_batch(_scalars(seed, n).reshape(-1).tobytes(), n)
    b, _ = eng.g2_mul_generator_batch(_scalars(seed + 1, n).reshape(-1).tobytes(), n)
    a, b = bytes(a), bytes(b)
    return [a[96 * i:96 * i + 96] for i in range(n)], [b[192 * i:192 * i + 192] for i in range(n)]


def _equation(xs, holds):
    """two pairs (aP, Q), (-P, bQ): their product is one exactly when b = a"""
    p = RC.g1_mul(RC.g1_generator(), P.rand_fr(xs).to_bytes(32, "big"))
    q = RC.g2_mul(RC.g2_generator(), P.rand_fr(xs).to_bytes(32, "big"))
    a = P.rand_fr(xs)
    b = a if holds else (a + 1) % P.R_ORDER
    return [RC.g1_mul(p, a.to_bytes(32, "big")), _neg1(p)], [q, RC.g2_mul(q, b.to_bytes(32, "big"))]


def _oracle_item(g1s, g2s, skip=None):
    keep = [k for k in range(len(g1s)) if not (skip and skip[k])]
    if not keep:
        return ONE
    ok, v = RC.final_exponentiation(RC.miller_loop(b"".join(g1s[k] for k in keep), b"".join(g2s[k] for k in keep), len(keep)))
    assert ok
    return v


def _oracle(g1s, g2s, sizes, skip=None):
    out, at = [], 0
    for n in sizes:
        out.append(_oracle_item(g1s[at:at + n], g2s[at:at + n], skip[at:at + n] if skip is not None else None))
        at += n
    return np.array(out, dtype=np.uint64).reshape(len(sizes), 72)


def _check(vals, one, want, what=""):
    assert vals.shape == want.shape, what
    for j in range(want.shape[0]):
        assert np.array_equal(vals[j], want[j]), (what, j)
        assert one[j] == (1 if np.array_equal(want[j], ONE) else 0), (what, j)


# segment lengths 0, 1, 2, 3, 4, 5, 8, 17 and 64 in mixed order; the two-pair segments at the end are an equation that holds and one that does not
SIZES = [3, 0, 1, 64, 2, 17, 0, 5, 8, 4, 1, 2, 2, 0]


@pytest.fixture(scope="module")
def ragged(eng):
    n = sum(SIZES) - 4
    g1s, g2s = _points(eng, n, 11)
    xs = P.XORShift(77)
    for holds in (True, False):
        a, b = _equation(xs, holds)
        g1s += a; g2s += b
    want = _oracle(g1s, g2s, SIZES)
    assert np.array_equal(want[-3], ONE) and not np.array_equal(want[-2], ONE) and np.array_equal(want[-1], ONE) and np.array_equal(want[1], ONE)
    return g1s, g2s, eng.seg_offsets(SIZES), want


def test_ragged_segments_match_the_oracle(eng, ragged):
    g1s, g2s, off, want = ragged
    _defaults(eng)
    vals, one = eng.pairing_product_batch(b"".join(g1s), b"".join(g2s), off)
    _check(vals, one, want, "ragged")
    assert one.tolist() == [0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1]


def test_single_pair_segments_equal_pairing_batch(eng):
    _defaults(eng)
    n = 70
    g1s, g2s = _points(eng, n, 21)
    a, b = b"".join(g1s), b"".join(g2s)
    vals, one = eng.pairing_product_batch(a, b, eng.seg_offsets([1] * n))
    assert np.array_equal(vals, eng.pairing_batch(a, b, n))
    assert not one.any()


def _fold(values):
    acc = ONE
    for v in values:
        acc = RC.fq12_mul(acc, v)
    return acc


LONG = [2500, 1, 1300, 0, 296]


@pytest.fixture(scope="module")
def long_case(eng):
    _defaults(eng)
    n = sum(LONG)
    g1s, g2s = _points(eng, n, 31)
    a, b = b"".join(g1s), b"".join(g2s)
    single = eng.pairing_batch(a, b, n)
    want, at = [], 0
    for k in LONG:
        want.append(_fold(single[at:at + k])); at += k
    return a, b, eng.seg_offsets(LONG), np.array(want, dtype=np.uint64).reshape(len(LONG), 72)


def test_long_segments_equal_the_fold_of_single_pairings(eng, long_case):
    a, b, off, want = long_case
    _defaults(eng)
    vals, one = eng.pairing_product_batch(a, b, off)      # 2 500 pairs at 8 a chunk: 313 partials, then 40, then 5 -- two fold passes
    _check(vals, one, want, "long")


def test_chunk_size_does_not_change_the_result(eng, long_case, ragged):
    a, b, off, want = long_case
    g1s, g2s, roff, rwant = ragged
    try:
        for K in (2, 3, 0, 1024, 1 << 20):                # K = 2: 2 500 -> 1 250 -> 625 -> ... -> 2: ten fold passes
            eng.set_option("segsum_chunk", K)
            vals, one = eng.pairing_product_batch(a, b, off)
            _check(vals, one, want, "long K=%d" % K)
            vals, one = eng.pairing_product_batch(b"".join(g1s), b"".join(g2s), roff)
            _check(vals, one, rwant, "ragged K=%d" % K)
    finally:
        eng.set_option("segsum_chunk", 0)


def test_infinity(eng):
    _defaults(eng)
    sizes = [0, 4, 4, 0, 2, 5, 1, 0]                      # empty segments first, in the middle and last
    n = sum(sizes)
    g1s, g2s = _points(eng, n, 41)
    flags = np.zeros(n, dtype=np.uint8)
    flags[1] = 1                                          # P flagged
    flags[2] = 2                                          # Q flagged
    flags[4] = 3                                          # both
    g1s[5] = bytes(96)                                    # all-zero records: P, then Q, then both
    g2s[6] = bytes(192)
    flags[8] = 1; flags[9] = 2                            # a segment (positions 8, 9) made only of skipped pairs
    g1s[11] = bytes(96); g2s[11] = bytes(192)
    flags[15] = 2                                         # the single-pair segment, skipped
    skip = flags.astype(bool)
    skip[[5, 6, 11]] = True
    want = _oracle(g1s, g2s, sizes, list(skip))
    assert np.array_equal(want[4], ONE) and np.array_equal(want[6], ONE)
    vals, one = eng.pairing_product_batch(b"".join(g1s), b"".join(g2s), eng.seg_offsets(sizes), flags)
    _check(vals, one, want, "infinity, affine")
    assert one.tolist() == [1, 0, 0, 1, 1, 0, 1, 1]
    # the in-memory form: z = 0 (whatever x and y hold) and the reference's G?ProjectiveZero
    xs = P.XORShift(5)
    j1 = [g1_to_jac(None) if g1s[k] == bytes(96) else jac1(xs, g1s[k]) for k in range(n)]
    j2 = [g2_to_jac(None) if g2s[k] == bytes(192) else jac2(xs, g2s[k]) for k in range(n)]
    for k in range(n):
        if flags[k] & 1:
            j1[k] = g1_to_jac(g1s[k], 0)
        if flags[k] & 2:
            j2[k] = g2_to_jac(g2s[k], (0, 0))
    jv, jo = eng.pairing_product_batch_jac(b"".join(j1), b"".join(j2), eng.seg_offsets(sizes))
    _check(jv, jo, want, "infinity, in-memory")
    # no pairs at all: every item is one
    vals, one = eng.pairing_product_batch(b"", b"", eng.seg_offsets([0, 0, 0]))
    assert one.tolist() == [1, 1, 1] and all(np.array_equal(v, ONE) for v in vals)


def _profiled(eng, fn):
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


def test_every_layout_gives_the_same_bytes(eng, ragged):
    g1s, g2s, off, want = ragged                         # np = 109 pairs, m = 14 items
    a, b = b"".join(g1s), b"".join(g2s)
    # (thresholds, the Miller kernel, the final-exponentiation kernel) -- the stages' layouts follow the sizes np and m
    combos = [
        (lambda: (eng.set_row_threshold(1, 1 << 20),), "k_miller1h_row", "k_final_exp_row"),
        (lambda: (eng.set_row_threshold(0, 0), eng.set_latency_threshold(0), eng.set_quad_threshold(1 << 20)), "k_miller1h_quad", "k_final_exp_quad"),
        (lambda: (eng.set_row_threshold(0, 0), eng.set_latency_threshold(0), eng.set_quad_threshold(0)), "k_miller1h_pair", "k_final_exp_pair"),
        (lambda: (eng.set_row_threshold(0, 0), eng.set_latency_threshold(8192), eng.set_quad_threshold(0)), "k_lat:miller1raw", "k_lat:finalexp1"),
        (lambda: (eng.set_row_threshold(100, 1 << 20),), "k_miller1h_row", "k_lat:finalexp1"),            # np in the row range, m below it
        (lambda: (eng.set_row_threshold(1, 50), eng.set_latency_threshold(0), eng.set_quad_threshold(1 << 20)), "k_miller1h_quad", "k_final_exp_row"),
        (lambda: (eng.set_row_threshold(1, 50), eng.set_latency_threshold(8192), eng.set_quad_threshold(0)), "k_lat:miller1raw", "k_final_exp_row"),
    ]
    try:
        for setup, miller, fe in combos:
            _defaults(eng)
            setup()
            (vals, one), prof = _profiled(eng, lambda: eng.pairing_product_batch(a, b, off))
            assert miller in prof and fe in prof and "k_fq12_seg_prod_row" in prof and "k_fq12_is_one_m384" in prof, (miller, fe, sorted(prof))
            _check(vals, one, want, miller + " + " + fe)
    finally:
        _defaults(eng)


def _t(b):
    import torch
    a = np.frombuffer(bytes(b), dtype=np.uint8).copy() if not isinstance(b, np.ndarray) else np.ascontiguousarray(b).view(np.uint8).reshape(-1).copy()
    if a.size == 0:
        a = np.zeros(8, dtype=np.uint8)
    return torch.from_numpy(a).to(torch.device("cuda", 0))


def test_the_four_forms_agree(eng, ragged):
    import torch
    _defaults(eng)
    g1s, g2s, off, want = ragged
    g1s, g2s = list(g1s), list(g2s)
    n, m = len(g1s), len(off) - 1
    flags = np.zeros(n, dtype=np.uint8)
    flags[0] = 1; flags[70] = 2; g1s[3] = bytes(96)       # a few skipped pairs as well
    a, b = b"".join(g1s), b"".join(g2s)
    hv, ho = eng.pairing_product_batch(a, b, off, flags)
    skip = flags.astype(bool); skip[3] = True
    _check(hv, ho, _oracle(g1s, g2s, SIZES, list(skip)), "host affine")
    xs = P.XORShift(9)
    j1 = [g1_to_jac(g1s[k], 0) if flags[k] & 1 else g1_to_jac(None) if g1s[k] == bytes(96) else jac1(xs, g1s[k]) for k in range(n)]
    j2 = [g2_to_jac(g2s[k], (0, 0)) if flags[k] & 2 else jac2(xs, g2s[k]) for k in range(n)]
    jv, jo = eng.pairing_product_batch_jac(b"".join(j1), b"".join(j2), off)
    assert np.array_equal(jv, hv) and np.array_equal(jo, ho)
    d_off = _t(off)
    for jac in (False, True):
        d1, d2 = (_t(b"".join(j1)), _t(b"".join(j2))) if jac else (_t(a), _t(b))
        keep1, keep2 = d1.clone(), d2.clone()
        d_fl = _t(flags)
        d_out = torch.zeros(m * 576, dtype=torch.uint8, device=d1.device)
        d_one = torch.full((m,), 7, dtype=torch.uint8, device=d1.device)
        eng.pairing_product_batch_dev(d1.data_ptr(), d2.data_ptr(), n, d_off.data_ptr(), m, d_out.data_ptr(), d_one.data_ptr(),
                                      d_inf_flags=0 if jac else d_fl.data_ptr(), jac=jac)
        assert np.array_equal(d_out.cpu().numpy().view(np.uint64).reshape(m, 72), hv), jac
        assert np.array_equal(d_one.cpu().numpy(), ho), jac
        assert torch.equal(d1, keep1) and torch.equal(d2, keep2), "the caller's points are left as they were"
        # either output alone, on a stream of the caller's
        st = torch.cuda.Stream(device=d1.device)
        d_one.fill_(7); d_out.zero_()
        eng.pairing_product_batch_dev(d1.data_ptr(), d2.data_ptr(), n, d_off.data_ptr(), m, 0, d_one.data_ptr(),
                                      d_inf_flags=0 if jac else d_fl.data_ptr(), stream=st.cuda_stream, jac=jac)
        assert np.array_equal(d_one.cpu().numpy(), ho), jac
        eng.pairing_product_batch_dev(d1.data_ptr(), d2.data_ptr(), n, d_off.data_ptr(), m, d_out.data_ptr(), 0,
                                      d_inf_flags=0 if jac else d_fl.data_ptr(), stream=st.cuda_stream, jac=jac)
        assert np.array_equal(d_out.cpu().numpy().view(np.uint64).reshape(m, 72), hv), jac
    # the host form with one output only
    from bls_amd import _native
    lib = _native.load()
    u8 = np.frombuffer(a, dtype=np.uint8); v8 = np.frombuffer(b, dtype=np.uint8)
    only = np.full(m, 7, dtype=np.uint8)
    p8, p64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64)
    rc = lib.blsmi_pairing_product_batch(u8.ctypes.data_as(p8), v8.ctypes.data_as(p8), flags.ctypes.data_as(p8), ctypes.c_size_t(n),
                                         off.ctypes.data_as(p64), ctypes.c_size_t(m), None, only.ctypes.data_as(p8))
    assert rc == 0 and np.array_equal(only, ho)


def test_dev_forms_refuse_bad_offsets(eng):
    import torch
    _defaults(eng)
    g1s, g2s = _points(eng, 4, 51)
    d1, d2 = _t(b"".join(g1s)), _t(b"".join(g2s))
    j1, j2 = _t(b"".join(g1_to_jac(p) for p in g1s)), _t(b"".join(g2_to_jac(q) for q in g2s))
    d_out = torch.zeros(3 * 576, dtype=torch.uint8, device=d1.device)
    d_one = torch.zeros(3, dtype=torch.uint8, device=d1.device)
    for bad in ([1, 2, 4], [0, 3, 2, 4], [0, 2, 3], [0, 2, 5]):
        d_off = _t(np.array(bad, dtype=np.uint64))
        for jac in (False, True):
            with pytest.raises(eng.BlsmiError, match="bad argument"):
                eng.pairing_product_batch_dev((j1 if jac else d1).data_ptr(), (j2 if jac else d2).data_ptr(), 4, d_off.data_ptr(), len(bad) - 1,
                                              d_out.data_ptr(), d_one.data_ptr(), jac=jac)
    # and the library still serves a good call afterwards
    d_off = _t(np.array([0, 1, 4], dtype=np.uint64))
    eng.pairing_product_batch_dev(d1.data_ptr(), d2.data_ptr(), 4, d_off.data_ptr(), 2, d_out.data_ptr(), d_one.data_ptr())
    hv, ho = eng.pairing_product_batch(b"".join(g1s), b"".join(g2s), [0, 1, 4])
    assert np.array_equal(d_out.cpu().numpy()[:2 * 576].view(np.uint64).reshape(2, 72), hv) and np.array_equal(d_one.cpu().numpy()[:2], ho)


def test_two_threads_with_different_shapes(eng, ragged, long_case):
    _defaults(eng)
    g1s, g2s, roff, rwant = ragged
    a, b, loff, lwant = long_case
    ra, rb = b"".join(g1s), b"".join(g2s)
    errs = []

    def work(x, y, off, want, rounds, what):
        try:
            for _ in range(rounds):
                vals, one = eng.pairing_product_batch(x, y, off)
                _check(vals, one, want, what)
        except Exception as e:  # noqa: BLE001 -- reported by the main thread
            errs.append((what, repr(e)))

    th = [threading.Thread(target=work, args=(ra, rb, roff, rwant, 6, "ragged")), threading.Thread(target=work, args=(a, b, loff, lwant, 3, "long"))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
