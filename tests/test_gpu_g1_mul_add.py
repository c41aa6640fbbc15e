"""-m gpu: the G1 lift out = A + (k mod r) * B (blsmi 0.20: blsmi_g1_mul_add_batch[_dev], k_g1_mul_add_glv), byte for byte against the oracle's
ladder and sum, in both forms.  Every call carries the rows where the group law leaves its common path -- A, B or both at infinity, k = 0, r
and 1 with A = B (the final addition is a doubling), A = -k B (the all-zero record and out_inf = 1), k = r - 1 and 2^256 - 1 -- and n runs
over the sizes around a wave (1, 63, 64, 65) and several workgroups (257), so that the clamped lanes behind n in the last wave are there."""
import numpy as np
import pytest

from gpu_common import P
from kzg_cases import INF, R, g1_mul, g1_neg, g1_sum
from oracle import refcpu as RC
from test_gpu_pprod_rlc import _defaults, _t

pytestmark = pytest.mark.gpu

NS = (1, 63, 64, 65, 257)
TOP = 2 ** 256 - 1


@pytest.fixture(scope="module")
def eng():
    from bls_amd import engine
    engine.init(0)
    yield engine
    _defaults(engine)


@pytest.fixture(scope="module")
def kzg(eng):
    from bls_amd import kzg
    return kzg


def _special_rows(xs):
    """(A, B, k) of the rows every call carries"""
    g = RC.g1_generator()
    pt = lambda: g1_mul(g, P.rand_fr(xs))                                        # noqa: E731
    rows = [(INF, pt(), P.rand_fr(xs)), (pt(), INF, P.rand_fr(xs)), (INF, INF, P.rand_fr(xs))]
    for k in (0, R, 1):
        p = pt()
        rows.append((p, p, k))                                                   # A = B: k = 1 makes the final addition a doubling
    for k in (P.rand_fr(xs), R - 1, TOP):
        b = pt()
        rows.append((g1_neg(g1_mul(b, k)), b, k))                                # A = -k B: infinity
    rows += [(pt(), pt(), R - 1), (pt(), pt(), TOP)]
    return rows


@pytest.fixture(scope="module")
def rows():
    """257 rows with the oracle's results, computed once: the special rows first and again at the end, random rows between"""
    xs = P.XORShift(2020)
    g = RC.g1_generator()
    special = _special_rows(xs)
    mid = [(g1_mul(g, P.rand_fr(xs)), g1_mul(g, P.rand_fr(xs)), P.rand_int(xs, 1 << 256)) for _ in range(257 - 2 * len(special))]
    all_rows = special + mid + special[::-1]
    want = [g1_sum([a, g1_mul(b, k)]) for a, b, k in all_rows]
    assert want[0] != INF and want[1] != INF and want[2] == INF and want[3] == all_rows[3][0] and want[4] == all_rows[4][0]
    assert want[5] == g1_mul(all_rows[5][0], 2) and want[6:9] == [INF] * 3 and len(all_rows) == 257
    return all_rows, want, len(special)


def _pick(rows, n):
    """n rows of the corpus that keep the special ones: all of them from 22 rows up, the first and the last otherwise"""
    all_rows, want, ns = rows
    if n == 1:
        idx = [6]                                                                # a lone item whose result is infinity
    else:
        idx = list(range(n - n // 2)) + list(range(257 - n // 2, 257))
    return [all_rows[i] for i in idx], [want[i] for i in idx]


def _pack(picked, a_stride=96, b_stride=96):
    n = len(picked)
    def lay(col, stride):                                                         # noqa: E306
        if stride == 0:
            return picked[0][col]
        buf = bytearray(b"\x5a" * (stride * (n - 1) + 96))
        for j, row in enumerate(picked):
            buf[stride * j:stride * j + 96] = row[col]
        return bytes(buf)
    return lay(0, a_stride), lay(1, b_stride), b"".join(k.to_bytes(32, "big") for _, _, k in picked)


def _check(out, inf, want):
    got = [bytes(r) for r in np.asarray(out, dtype=np.uint8).reshape(-1, 96)]
    assert got == want                                                           # byte for byte; infinity is the all-zero record
    assert [bool(x) for x in inf] == [w == INF for w in want]


@pytest.mark.parametrize("n", NS)
def test_host_form_against_the_oracle(eng, kzg, rows, n):
    _defaults(eng)
    picked, want = _pick(rows, n)
    a, b, k = _pack(picked)
    out, inf = kzg.g1_mul_add_batch(a, b, k, n)
    _check(out, inf, want)


def test_every_special_row_alone(eng, kzg, rows):
    """n = 1 for each special row: one live lane, 63 clamped ones repeating it"""
    all_rows, want, ns = rows
    for i in range(ns):
        a, b, k = _pack([all_rows[i]])
        out, inf = kzg.g1_mul_add_batch(a, b, k, 1)
        _check(out, inf, [want[i]])


def test_strides_other_than_96(eng, kzg, rows):
    _defaults(eng)
    picked, want = _pick(rows, 65)
    a, b, k = _pack(picked, 128, 192)
    out, inf = kzg.g1_mul_add_batch(a, b, k, 65, a_stride=128, b_stride=192)
    _check(out, inf, want)
    # one common multiplicand (stride 0), and one common summand
    all_rows, _, ns = rows
    some = all_rows[ns:ns + 5]
    b0 = some[0][1]
    common_b = [(r[0], b0, r[2]) for r in some]
    a, b, k = _pack(common_b, 96, 0)
    out, inf = kzg.g1_mul_add_batch(a, b, k, 5, b_stride=0)
    _check(out, inf, [g1_sum([r[0], g1_mul(b0, r[2])]) for r in common_b])
    a0 = some[1][0]
    common_a = [(a0, r[1], r[2]) for r in some]
    a, b, k = _pack(common_a, 0, 100)
    out, inf = kzg.g1_mul_add_batch(a, b, k, 5, a_stride=0, b_stride=100)
    _check(out, inf, [g1_sum([a0, g1_mul(r[1], r[2])]) for r in common_a])


@pytest.mark.parametrize("n", NS)
def test_dev_form_word_aligned_and_inputs_untouched(eng, kzg, rows, n):
    """the device-pointer form over buffers at an address = 4 mod 16 (a stride of 96 and one of 104), on stream 0 and on a side stream"""
    import torch
    _defaults(eng)
    picked, want = _pick(rows, n)
    a, b, k = _pack(picked, 96, 104)
    shifted = []
    for x in (a, b, k):
        buf = _t(b"\xa5" * 4 + x + b"\xa5" * 12)
        shifted.append((buf, buf[4:4 + len(x)]))
        assert shifted[-1][1].data_ptr() % 16 == 4
    keep = [buf.clone() for buf, _ in shifted]
    st = torch.cuda.Stream(device=keep[0].device)
    for stream in (0, st.cuda_stream):
        d_out = torch.full((96 * n + 16,), 7, dtype=torch.uint8, device=keep[0].device)
        d_inf = torch.full((n,), 7, dtype=torch.uint8, device=keep[0].device)
        kzg.g1_mul_add_batch_dev(shifted[0][1].data_ptr(), 96, shifted[1][1].data_ptr(), 104, shifted[2][1].data_ptr(), d_out[4:].data_ptr(), d_inf.data_ptr(), n, stream=stream)
        out = d_out.cpu().numpy()
        assert out[:4].tolist() == [7] * 4 and out[4 + 96 * n:].tolist() == [7] * 12     # nothing written outside the n records
        _check(out[4:4 + 96 * n], d_inf.cpu().numpy(), want)
    for (buf, _), kept in zip(shifted, keep):
        assert torch.equal(buf, kept), "the caller's device buffers are byte-identical afterwards"
