"""-m gpu: the weighted segmented fold of scalars mod r (blsmi 0.19: blsmi_fr_wsum_segmented_u64[_dev], k_fr_wsum_u64 + k_fr_wsum_fold)
against Python big integers, byte for byte, in the host and the device-pointer form.  tests/test_groth16_cpu.py runs the same arithmetic
(bls_amd/csrc/fr_fold.h) natively."""
import numpy as np
import pytest

from groth16_cases import R
from oracle import pyref as P
from test_gpu_pprod_rlc import _t

pytestmark = pytest.mark.gpu

TOP = (1 << 64) - 1
LENGTHS = (0, 1, 2, 63, 0, 64, 65, 257, 0)                                       # an empty segment first, in the middle and last


@pytest.fixture(scope="module")
def eng():
    from bls_amd import engine
    engine.init(0)
    return engine


def _want(rows, weights, off, ncol):
    out = []
    for lo, hi in zip(off[:-1], off[1:]):
        out.append([sum(weights[lo:hi]) % R] + [sum(weights[j] * rows[j][i] for j in range(lo, hi)) % R for i in range(ncol)])
    return out


def _bytes(rows):
    return b"".join(v.to_bytes(32, "big") for row in rows for v in row)


def _ints(out):
    return [[int.from_bytes(bytes(cell), "big") for cell in seg] for seg in out]


def _check(eng, rows, weights, off, ncol, dev=True):
    want = _want(rows, weights, off, ncol)
    assert all(v < R for seg in want for v in seg)
    got = eng.fr_wsum_segmented_u64(_bytes(rows), ncol, weights, off)
    assert got.shape == (len(off) - 1, ncol + 1, 32)
    assert _ints(got) == want                                                    # every output byte, every output below r
    if dev:
        import torch
        d_v, d_w, d_off = _t(_bytes(rows)), _t(np.asarray(weights, dtype=np.uint64)), _t(np.asarray(off, dtype=np.uint64))
        keep = [t.clone() for t in (d_v, d_w, d_off)]
        d_out = torch.full((32 * (ncol + 1) * (len(off) - 1) + 8,), 0xa5, dtype=torch.uint8, device=d_v.device)
        eng.fr_wsum_segmented_u64_dev(d_v.data_ptr(), ncol, d_w.data_ptr(), d_off.data_ptr(), len(off) - 1, d_out.data_ptr())
        raw = d_out.cpu().numpy()
        assert raw[-8:].tolist() == [0xa5] * 8, "nothing is written behind the outputs"
        assert _ints(raw[:-8].reshape(len(off) - 1, ncol + 1, 32)) == want
        for t, k in zip((d_v, d_w, d_off), keep):
            assert torch.equal(t, k), "the caller's device buffers are byte-identical afterwards"


@pytest.mark.parametrize("ncol", [1, 2, 3, 8, 17])
def test_segments_of_every_length_in_one_call(eng, ncol):
    """lengths 0, 1, 2, 63, 64, 65, 257 with empty segments first, last and in the middle; random values below 2^256 with the extreme ones
    (0, r - 1, r, 2^256 - 1) and the extreme weights (2^64 - 1, 1, 0) among them"""
    xs = P.XORShift(100 + ncol)
    n = sum(LENGTHS)
    off = [0]
    for length in LENGTHS:
        off.append(off[-1] + length)
    extreme = (0, R - 1, R, 2 ** 256 - 1)
    rows = [[extreme[(j + i) % 4] if (j * ncol + i) % 5 == 0 else P.rand_int(xs, 1 << 256) for i in range(ncol)] for j in range(n)]
    weights = [(TOP, 1, 0)[j % 7] if j % 7 < 3 else P.rand_int(xs, 1 << 64) for j in range(n)]
    _check(eng, rows, weights, off, ncol)


@pytest.mark.parametrize("value", [R - 1, 2 ** 256 - 1, 0])
def test_the_longest_carries(eng, value):
    """every value r - 1 / 2^256 - 1 under weight 2^64 - 1: every lane's accumulator and every LDS addition carries through all its words"""
    for ncol in (1, 3):
        n = 257
        _check(eng, [[value] * ncol] * n, [TOP] * n, [0, n], ncol, dev=False)
    _check(eng, [[value] * 2] * 4, [0] * 4, [0, 4], 2, dev=False)                # zero weights only
    _check(eng, [[value, value]], [TOP], [0, 1], 2, dev=False)                   # one row


@pytest.mark.parametrize("n,ncol", [(70000, 1), (9000, 8)])
def test_a_segment_that_spans_workgroups(eng, n, ncol):
    """one segment longer than a workgroup's share (4 096 rows of one column, 448 rows of eight), between two short ones"""
    rng = np.random.default_rng(7 * ncol)
    raw = rng.integers(0, 256, size=(n + 5, ncol, 32), dtype=np.uint8)
    raw[::97] = 0xff                                                             # rows of 2^256 - 1 among them
    w = rng.integers(0, 1 << 64, size=n + 5, dtype=np.uint64)
    w[::101] = TOP
    rows = [[int.from_bytes(raw[j, i].tobytes(), "big") for i in range(ncol)] for j in range(n + 5)]
    weights = [int(x) for x in w]
    off = [0, 2, 2 + n, n + 5]
    want = _want(rows, weights, off, ncol)
    got = eng.fr_wsum_segmented_u64(raw.tobytes(), ncol, weights, off)
    assert _ints(got) == want
    import torch
    d_v, d_w, d_off = _t(raw.tobytes()), _t(w), _t(np.asarray(off, dtype=np.uint64))
    d_out = torch.zeros(32 * (ncol + 1) * 3, dtype=torch.uint8, device=d_v.device)
    eng.fr_wsum_segmented_u64_dev(d_v.data_ptr(), ncol, d_w.data_ptr(), d_off.data_ptr(), 3, d_out.data_ptr())
    assert _ints(d_out.cpu().numpy().reshape(3, ncol + 1, 32)) == want


def test_values_that_are_only_word_aligned_and_no_column(eng):
    """the caller's scalars 4 bytes into a buffer: read byte by byte, the same outputs; ncol = 0: the weights' sums alone"""
    import torch
    xs = P.XORShift(5)
    rows = [[P.rand_int(xs, 1 << 256) for _ in range(3)] for _ in range(70)]
    weights = [P.rand_int(xs, 1 << 64) for _ in range(70)]
    off = [0, 1, 70]
    want = _want(rows, weights, off, 3)
    buf = _t(b"\xa5" * 4 + _bytes(rows) + b"\xa5" * 12)
    d_v = buf[4:4 + 32 * 3 * 70]
    assert d_v.data_ptr() % 16 == 4
    d_w, d_off = _t(np.asarray(weights, dtype=np.uint64)), _t(np.asarray(off, dtype=np.uint64))
    d_out = torch.zeros(32 * 4 * 2, dtype=torch.uint8, device=buf.device)
    eng.fr_wsum_segmented_u64_dev(d_v.data_ptr(), 3, d_w.data_ptr(), d_off.data_ptr(), 2, d_out.data_ptr())
    assert _ints(d_out.cpu().numpy().reshape(2, 4, 32)) == want
    got = eng.fr_wsum_segmented_u64(b"", 0, weights, off)
    assert _ints(got) == [[weights[0] % R], [sum(weights[1:]) % R]]
