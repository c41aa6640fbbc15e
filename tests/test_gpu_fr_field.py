"""-m gpu: products and inverses mod r on the device (blsmi 0.21: blsmi_fr_mul_batch[_dev], blsmi_fr_inv_batch[_dev], k_fr_mul, k_fr_inv)
against Python integers, on the grid of edge operands tests/test_fr_eval_cpu.py runs fr.h on natively."""
import numpy as np
import pytest

from fr_eval_cases import EDGE_OPERANDS, R, grid_pairs
from kzg_cases import scalar_bytes
from test_gpu_pprod_rlc import _t

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 257)                                                     # a partly filled wave, a full one, one lane over; a second workgroup


@pytest.fixture(scope="module")
def fr():
    from bls_amd import engine, fr
    engine.init(0)
    return fr


@pytest.fixture(scope="module")
def grid():
    pairs = grid_pairs(300, 22)
    a, b = [p[0] for p in pairs], [p[1] for p in pairs]
    return a, b, [x * y % R for x, y in zip(a, b)], [pow(x % R, R - 2, R) for x in a]


def _ints(out):
    return [int.from_bytes(bytes(row), "big") for row in np.asarray(out).reshape(-1, 32)]


def _unaligned(data):
    """the same bytes at an odd address"""
    buf = np.full(len(data) + 2, 0x5a, dtype=np.uint8)
    off = 1 if buf.ctypes.data % 2 == 0 else 2
    a = buf[off:off + len(data)]
    a[:] = np.frombuffer(data, dtype=np.uint8)
    assert a.ctypes.data % 2 == 1
    return a


def test_products_and_inverses_on_the_grid(fr, grid):
    a, b, prod, inv = grid
    assert len(a) == len(EDGE_OPERANDS) ** 2 + 300
    assert _ints(fr.mul_batch(scalar_bytes(a), scalar_bytes(b))) == prod
    assert _ints(fr.inv_batch(scalar_bytes(a))) == inv
    assert _ints(fr.inv_batch(scalar_bytes([0, R, 2 * R, 1, R + 1, R - 1]))) == [0, 0, 0, 1, 1, R - 1]   # the inverse of 0 mod r is 0


@pytest.mark.parametrize("n", SIZES)
def test_sizes_in_both_forms(fr, grid, n):
    import torch
    a, b, prod, inv = (v[-n:] for v in grid)                                     # the random tail, and edge pairs before it at 257
    ab, bb = scalar_bytes(a), scalar_bytes(b)
    assert _ints(fr.mul_batch(_unaligned(ab), _unaligned(bb))) == prod           # host buffers at an odd address
    assert _ints(fr.inv_batch(_unaligned(ab))) == inv
    da, db = _t(ab), _t(bb)
    keep = (da.clone(), db.clone())
    st = torch.cuda.Stream(device=da.device)
    for stream in (0, st.cuda_stream):
        out = torch.full((32 * n + 32,), 0xa5, dtype=torch.uint8, device=da.device)
        fr.mul_batch_dev(da.data_ptr(), db.data_ptr(), out.data_ptr(), n, stream=stream)
        assert _ints(out[:32 * n].cpu().numpy()) == prod and bytes(out[32 * n:].cpu().numpy()) == b"\xa5" * 32   # nothing behind element n - 1
        out = torch.full((32 * n + 32,), 0xa5, dtype=torch.uint8, device=da.device)
        fr.inv_batch_dev(da.data_ptr(), out.data_ptr(), n, stream=stream)
        assert _ints(out[:32 * n].cpu().numpy()) == inv and bytes(out[32 * n:].cpu().numpy()) == b"\xa5" * 32
    assert torch.equal(da, keep[0]) and torch.equal(db, keep[1])                 # the inputs stay untouched


def test_dev_buffers_that_are_only_word_aligned(fr, grid):
    a, b, prod, inv = (v[:65] for v in grid)
    bufs = []
    for x in (scalar_bytes(a), scalar_bytes(b), bytes(32 * 65)):
        t = _t(b"\xa5" * 4 + x + b"\xa5" * 12)
        bufs.append((t, t[4:4 + len(x)]))
        assert bufs[-1][1].data_ptr() % 16 == 4
    (_, da), (_, db), (whole, out) = bufs
    fr.mul_batch_dev(da.data_ptr(), db.data_ptr(), out.data_ptr(), 65)
    assert _ints(out.cpu().numpy()) == prod
    fr.inv_batch_dev(da.data_ptr(), out.data_ptr(), 65)
    assert _ints(out.cpu().numpy()) == inv
    assert bytes(whole[:4].cpu().numpy()) == b"\xa5" * 4 and bytes(whole[-12:].cpu().numpy()) == b"\xa5" * 12
    assert fr.mul_batch(b"", b"").shape == (0, 32) and fr.inv_batch(b"").shape == (0, 32)
