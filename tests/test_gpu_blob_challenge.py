"""-m gpu: the Fiat-Shamir challenge of blob proofs on the device (blsmi 0.23: blsmi_kzg_blob_challenge_batch[_dev]; k_kzg_fs_split, and
k_kzg_fs_lane behind blsmi_debug_kzg_blob_challenge_form_dev), byte for byte against the model of tests/blob_wire_cases.py (hashlib; held
against its block-wise restatement in tests/test_blob_wire_cpu.py).  Shapes: log2n 0 (its own tail), 1, 2 (no block whole in the blob yet),
4 and 8 times m = 1, 3, 63, 64, 65 and 130 -- the wave and workgroup edges of both forms --, and two blobs of 4 096."""
import random

import numpy as np
import pytest

from blob_wire_cases import INF48, QUOTIENT_CASES, challenge, digest, quotient_blob
from kzg_cases import R
from test_gpu_pprod_rlc import _t

pytestmark = pytest.mark.gpu

LOG2NS = (0, 1, 2, 4, 8)
MS = (1, 3, 63, 64, 65, 130)
FORMS = (1, 0)                                                                   # k_kzg_fs_split (the default), k_kzg_fs_lane


@pytest.fixture(scope="module")
def eng():
    from bls_amd import engine
    engine.init(0)
    return engine


@pytest.fixture(scope="module")
def kzg(eng):
    from bls_amd import kzg
    return kzg


@pytest.fixture(scope="module")
def batches():
    """{(k, m): (blob bytes, commitment bytes, expected z bytes)}: random bytes (nothing is decoded), the model computed once"""
    out = {}
    for k in LOG2NS + (12,):
        n = 1 << k
        for m in (MS if k != 12 else (2,)):
            rng = random.Random(100 * k + m)
            blobs = [rng.randbytes(32 * n) for _ in range(m)]
            comms = [rng.randbytes(48) for _ in range(m)]
            out[(k, m)] = (b"".join(blobs), b"".join(comms), b"".join(challenge(b, k, c).to_bytes(32, "big") for b, c in zip(blobs, comms)))
    return out


def _form(eng, d_polys, k, d_c, d_z, m, form, stream=0):
    eng._call("blsmi_debug_kzg_blob_challenge_form_dev", d_polys, k, d_c, d_z, m, form, stream)


@pytest.mark.parametrize("k", LOG2NS)
@pytest.mark.parametrize("m", MS)
def test_against_the_model_in_both_forms(eng, kzg, batches, k, m):
    import torch
    pb, cb, want = batches[(k, m)]
    assert bytes(kzg.blob_challenge_batch(pb, k, cb).reshape(-1)) == want, (k, m)     # the host form
    dp, dc = _t(pb), _t(cb)
    assert dp.data_ptr() % 16 == 0
    keep = (dp.clone(), dc.clone())
    st = torch.cuda.Stream(device=dp.device)
    for stream in (0, st.cuda_stream):
        dz = torch.full((32 * m + 32,), 0xa5, dtype=torch.uint8, device=dp.device)
        kzg.blob_challenge_batch_dev(dp.data_ptr(), k, dc.data_ptr(), dz.data_ptr(), m, stream=stream)
        got = bytes(dz.cpu().numpy())
        assert got[:32 * m] == want and got[32 * m:] == b"\xa5" * 32, (k, m, stream)   # and the guard bytes behind z
    for form in FORMS:
        dz = torch.full((32 * m + 32,), 0xa5, dtype=torch.uint8, device=dp.device)
        _form(eng, dp.data_ptr(), k, dc.data_ptr(), dz.data_ptr(), m, form, st.cuda_stream)
        got = bytes(dz.cpu().numpy())
        assert got[:32 * m] == want and got[32 * m:] == b"\xa5" * 32, (k, m, form)
    assert torch.equal(dp, keep[0]) and torch.equal(dc, keep[1])                 # the inputs stay untouched


@pytest.mark.parametrize("k,m", [(0, 65), (2, 3), (4, 65), (8, 3)])
def test_buffers_that_are_only_word_aligned(eng, batches, k, m):
    """every buffer 4 bytes off a 16-byte boundary: the blob's blocks are read word by word; the same challenges in both forms"""
    import torch
    pb, cb, want = batches[(k, m)]
    pw, cw = _t(b"\xa5" * 4 + pb + b"\xa5" * 12), _t(b"\xa5" * 4 + cb + b"\xa5" * 12)
    keep = (pw.clone(), cw.clone())
    assert pw[4:].data_ptr() % 16 == 4
    for form in FORMS:
        zw = _t(b"\xa5" * (4 + 32 * m + 12))
        _form(eng, pw[4:].data_ptr(), k, cw[4:].data_ptr(), zw[4:].data_ptr(), m, form)
        got = bytes(zw.cpu().numpy())
        assert got[4:4 + 32 * m] == want and got[:4] == b"\xa5" * 4 and got[4 + 32 * m:] == b"\xa5" * 12, (k, m, form)
    assert torch.equal(pw, keep[0]) and torch.equal(cw, keep[1])


def test_two_blobs_of_4096(eng, kzg, batches):
    pb, cb, want = batches[(12, 2)]
    assert bytes(kzg.blob_challenge_batch(pb, 12, cb).reshape(-1)) == want
    dp, dc = _t(pb), _t(cb)
    for form in FORMS:
        dz = _t(bytes(64))
        _form(eng, dp.data_ptr(), 12, dc.data_ptr(), dz.data_ptr(), 2, form)
        assert bytes(dz.cpu().numpy()) == want, form


def test_the_reduction_s_three_branches_and_bytes_that_decode_to_nothing(eng, kzg):
    blobs = [quotient_blob(v) for v, _ in QUOTIENT_CASES]
    assert [digest(b, 2, INF48) // R for b in blobs] == [0, 1, 2]
    want = b"".join(challenge(b, 2, INF48).to_bytes(32, "big") for b in blobs)
    assert bytes(kzg.blob_challenge_batch(b"".join(blobs), 2, INF48 * 3).reshape(-1)) == want
    dp, dc = _t(b"".join(blobs)), _t(INF48 * 3)
    for form in FORMS:
        dz = _t(bytes(96))
        _form(eng, dp.data_ptr(), 2, dc.data_ptr(), dz.data_ptr(), 3, form)
        assert bytes(dz.cpu().numpy()) == want, form
    for k in (0, 2, 4):                                                          # all 0xff: values >= r, a commitment that is no point -- only the digest sees them
        n = 1 << k
        want = challenge(b"\xff" * (32 * n), k, b"\xff" * 48).to_bytes(32, "big")
        assert bytes(kzg.blob_challenge_batch(b"\xff" * (32 * n * 2), k, b"\xff" * 96).reshape(-1)) == want * 2, k
    assert challenge(bytes(32 << 12), 12, INF48) == int.from_bytes(bytes(kzg.blob_challenge_batch(bytes(32 << 12), 12, INF48).reshape(-1)), "big")


def test_no_blob(kzg):
    z = kzg.blob_challenge_batch(b"", 12, b"")
    assert z.shape == (0, 32) and z.dtype == np.uint8
    kzg.blob_challenge_batch_dev(0, 12, 0, 0, 0)
