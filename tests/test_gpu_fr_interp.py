"""-m gpu: interpolation over a coset on the device (blsmi 0.22: blsmi_fr_coset_interp_batch[_dev]; k_fr_inv, k_fr_coset_interp), byte for
byte against the big-integer model of tests/cell_cases.py (held against p mod (X^n - h^n) and Horner's rule in tests/test_cell_cpu.py), in
both orders and both forms.  Shapes: n = 1 (256 items per workgroup, no stage), 2 (256 items), 4, 32, 64 (eight items), 512 (one item, two
elements per lane) and 1 024 (two tiles, the last stage in registers); one item, a few, 70 and 300 -- a ragged last workgroup at every
tiling."""
import random

import numpy as np
import pytest

from cell_cases import EDGE_SHIFTS, TOP, flags_of, interp, interp_fast, ints, vals_bytes
from fr_eval_cases import EDGE_OPERANDS, R
from kzg_cases import scalar_bytes
from test_gpu_pprod_rlc import _t
from test_gpu_pprod_rlc_segments import _segments

pytestmark = pytest.mark.gpu

LOGS = (0, 1, 2, 5, 6, 9, 10)
COUNTS = (1, 3, 70, 300)


@pytest.fixture(scope="module")
def eng():
    from bls_amd import engine
    engine.init(0)
    return engine


@pytest.fixture(scope="module")
def fr(eng):
    from bls_amd import fr
    return fr


def cell_values(kind, n, rng):
    if kind == 0:
        return [rng.randrange(R) for _ in range(n)]
    if kind == 1:
        return [rng.randrange(R)] * n                                            # constant: c_0 is the value, nothing else
    return [EDGE_OPERANDS[(i * 5 + rng.randrange(3)) % len(EDGE_OPERANDS)] if i % 2 == 0 else rng.getrandbits(256) for i in range(n)]


def model(cells, l, order, shifts):
    f = interp if l <= 2 else interp_fast                                        # (the fast form is held against the naive one on the CPU side)
    return [c for v, h in zip(cells, shifts) for c in f(v, l, order, h)]


_memo = {}


def batch(l, order, m):
    """(cells, shifts, expected coefficients, expected h^n, expected flags), the model computed once"""
    key = (l, order, m)
    if key not in _memo:
        rng = random.Random(1000 * l + 10 * m + order)
        n = 1 << l
        pool = [rng.randrange(1, R), *EDGE_SHIFTS, rng.getrandbits(256), rng.randrange(1, R)]
        cells = [cell_values(j % 3, n, rng) for j in range(m)]
        shifts = [pool[(j + j // len(pool)) % len(pool)] for j in range(m)]
        _memo[key] = (cells, shifts, model(cells, l, order, shifts), [pow(h % R, n, R) for h in shifts], [flags_of(v, h) for v, h in zip(cells, shifts)])
    return _memo[key]


@pytest.mark.parametrize("m", COUNTS)
@pytest.mark.parametrize("l", LOGS)
def test_against_the_model_in_both_orders_and_forms(fr, l, m):
    import torch
    n = 1 << l
    for order in (0, 1):
        cells, shifts, want, want_pow, want_fl = batch(l, order, m)
        vb, hb = vals_bytes(cells), scalar_bytes(shifts)
        co, sp, fl = fr.coset_interp_batch(vb, l, hb, order=order)
        assert co.shape == (m, n, 32) and ints(co) == want and ints(sp) == want_pow and fl.tolist() == want_fl, (l, order, m)
        co, sp, fl = fr.coset_interp_batch(vb, l, hb, order=order, shift_pow=False, flags=False)   # NULL for both
        assert ints(co) == want and sp is None and fl is None, (l, order, m)
        dv, dh = _t(vb), _t(hb)
        keep = (dv.clone(), dh.clone())
        st = torch.cuda.Stream(device=dv.device)
        for given, stream in ((True, 0), (False, st.cuda_stream)):
            dc = torch.full((32 * n * m + 32,), 0xa5, dtype=torch.uint8, device=dv.device)
            dp = torch.full((32 * m + 32,), 0xa5, dtype=torch.uint8, device=dv.device)
            df = torch.full((m + 4,), 7, dtype=torch.uint8, device=dv.device)
            fr.coset_interp_batch_dev(dv.data_ptr(), l, order, dh.data_ptr(), dc.data_ptr(), dp.data_ptr() if given else 0, df.data_ptr() if given else 0, m, stream=stream)
            assert ints(dc[:32 * n * m].cpu().numpy()) == want and bytes(dc[32 * n * m:].cpu().numpy()) == b"\xa5" * 32, (l, order, m)
            assert bytes(dp.cpu().numpy()) == (scalar_bytes(want_pow) if given else b"\xa5" * 32 * m) + b"\xa5" * 32, (l, order, m)
            assert df.cpu().numpy().tolist() == (want_fl if given else [7] * m) + [7] * 4, (l, order, m)
        assert torch.equal(dv, keep[0]) and torch.equal(dh, keep[1])             # the inputs stay untouched


def test_the_batches_hold_what_they_should():
    """the corpus itself: every kind of cell, every edge shift, every flag value, coefficients below r"""
    cells, shifts, want, want_pow, want_fl = batch(2, 1, 70)
    assert set(EDGE_SHIFTS) <= set(shifts) and set(want_fl) == {0, 1, 2, 3} and all(v < R for v in want + want_pow)
    assert any(v >= R for c in cells for v in c) and want[4 * 1 + 1:4 * 2] == [0, 0, 0] and want[4] == cells[1][0]   # the constant cell
    for j, h in enumerate(shifts):
        if h % R == 0:
            assert want[4 * j + 1:4 * j + 4] == [0, 0, 0] and want_pow[j] == 0 and want_fl[j] & 2


@pytest.mark.parametrize("l", LOGS)
def test_every_edge_shift(fr, l):
    """1, r - 1, r + 1, 0, r and 2^256 - 1 as the shift of a random cell, in both orders"""
    rng = random.Random(l)
    n, m = 1 << l, len(EDGE_SHIFTS)
    cells = [[rng.randrange(R) for _ in range(n)] for _ in range(m)]
    for order in (0, 1):
        want = model(cells, l, order, EDGE_SHIFTS)
        co, sp, fl = fr.coset_interp_batch(vals_bytes(cells), l, scalar_bytes(EDGE_SHIFTS), order=order)
        assert ints(co) == want and ints(sp) == [pow(h % R, n, R) for h in EDGE_SHIFTS] and fl.tolist() == [0, 0, 1, 2, 3, 1], (l, order)
        for j in (3, 4):                                                         # h = 0 mod r: c_0 the mean of the values, every other coefficient 0
            assert want[n * j:n * j + n] == [sum(cells[j]) * pow(n, -1, R) % R] + [0] * (n - 1)
    assert EDGE_SHIFTS == (1, R - 1, R + 1, 0, R, TOP)


@pytest.mark.parametrize("order", [0, 1])
def test_every_unit_vector(fr, order):
    """the value vector e_i for each of the n = 32 positions, one shift: a wrong position-to-root mapping or a wrong bit reversal shows here"""
    l, n, h = 5, 32, 0x1234567890abcdef1234567890abcdef
    cells = [[int(i == j) for i in range(n)] for j in range(n)]
    want = model(cells, l, order, [h] * n)
    assert len({tuple(want[n * j:n * j + n]) for j in range(n)}) == n
    co, _, fl = fr.coset_interp_batch(vals_bytes(cells), l, scalar_bytes([h] * n), order=order)
    assert ints(co) == want and not fl.any()


def test_buffers_that_are_only_word_aligned(fr):
    """device buffers 4 bytes off a 16-byte boundary: the values are read byte by byte, everything else by words -- the same bytes come out"""
    import torch
    for l, order, m in ((6, 1, 3), (9, 0, 3), (10, 1, 1)):
        cells, shifts, want, want_pow, want_fl = batch(l, order, m)
        n, vb = 1 << l, vals_bytes(cells)
        whole = _t(b"\xa5" * 4 + vb + b"\xa5" * 12)
        dv = whole[4:4 + len(vb)]
        assert dv.data_ptr() % 16 == 4
        hw = _t(b"\xa5" * 4 + scalar_bytes(shifts) + b"\xa5" * 12)
        cw = _t(b"\xa5" * (4 + 32 * n * m + 12))
        pw = _t(b"\xa5" * (4 + 32 * m + 12))
        df = _t(bytes(m))
        keep = (whole.clone(), hw.clone())
        fr.coset_interp_batch_dev(dv.data_ptr(), l, order, hw[4:].data_ptr(), cw[4:].data_ptr(), pw[4:].data_ptr(), df.data_ptr(), m)
        got = cw.cpu().numpy()
        assert ints(got[4:4 + 32 * n * m]) == want and bytes(got[:4]) == b"\xa5" * 4 and bytes(got[4 + 32 * n * m:]) == b"\xa5" * 12, (l, order)
        assert bytes(pw.cpu().numpy()) == b"\xa5" * 4 + scalar_bytes(want_pow) + b"\xa5" * 12 and df.cpu().numpy().tolist()[:m] == want_fl, (l, order)
        assert torch.equal(whole, keep[0]) and torch.equal(hw, keep[1])


def test_two_launches_whatever_m(eng, fr):
    """with profiling on a call names k_fr_inv and k_fr_coset_interp once each, in that order, for one cell and for 300 alike"""
    for l, order, m in ((6, 1, 1), (6, 1, 300), (10, 0, 3), (0, 0, 300)):
        cells, shifts, want, _, _ = batch(l, order, m)
        (co, _, _), names = _segments(eng, lambda: fr.coset_interp_batch(vals_bytes(cells), l, scalar_bytes(shifts), order=order))
        assert ints(co) == want
        assert [x for x in names if x.startswith("k_")] == ["k_fr_inv", "k_fr_coset_interp"], ((l, order, m), names)
