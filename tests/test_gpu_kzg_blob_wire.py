"""-m gpu: KZG blob batches from wire bytes (blsmi 0.23: blsmi_kzg_verify_blob_batch_wire[_dev]): the challenge, the decompression of the 2 m
points, the evaluation and blsmi_kzg_verify_batch behind them.  Verdicts, status, `combined` and `rechecked` against the big-integer model of
tests/blob_wire_cases.py, and the verdicts against kzg.verify_blob_batch given the model's z and the oracle's decompressed points, masked by
the status; every edge and every way of spoiling an item; both forms of the call."""
import pytest

from blob_wire_cases import EDGES, INF48, K, M, SEED, SPOILS, STATUS_OF_EDGE, WireCase
from test_gpu_pprod_rlc import _defaults, _pinned, _t

pytestmark = pytest.mark.gpu

BLOCKS = (0, 1, 8, 64)


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


@pytest.fixture(scope="module")
def cases():
    """every batch, computed once"""
    out = {"valid": WireCase(M, K, SEED, edge=EDGES)}
    for kind, spoil in SPOILS.items():
        out[kind] = WireCase(M, K, SEED, edge=EDGES, spoil=spoil)
    for kind, c in out.items():
        assert c.status == [STATUS_OF_EDGE.get(j, 0) for j in range(M)], kind
        assert c.verdicts() == [int(st == 0 and j not in SPOILS.get(kind, {})) for j, st in enumerate(c.status)], kind
    return out


def _wire(kzg, c, block, scalars, **kw):
    return kzg.verify_blob_batch_wire(c.srs_g1, c.srs_g2, c.poly_bytes, c.k, c.commitments48, c.proofs48, scalars=scalars, block=block, **kw)


@pytest.mark.parametrize("block", BLOCKS)
def test_verdicts_status_combined_and_rechecked(eng, kzg, cases, block):
    _defaults(eng)
    for kind, c in cases.items():
        want_ok, want_st, want_comb, want_nre = c.expect(block)
        ok, st, comb, nre = _wire(kzg, c, block, _pinned(M))
        assert (ok.tolist(), st.tolist(), comb, nre) == (want_ok, want_st, want_comb, want_nre), (kind, block)
        # the 0.21 call on the model's z and the oracle's points: the same verdicts once the status masks them
        ok0, nc0, _, _ = kzg.verify_blob_batch(c.srs_g1, c.srs_g2, c.poly_bytes, c.k, b"".join(c.C), b"".join(c.pi), c.z_bytes, order=1, scalars=_pinned(M), block=block)
        assert [int(o and s == 0) for o, s in zip(ok0.tolist(), c.status)] == ok.tolist() and nc0.tolist() == c.noncanon, (kind, block)
    c = cases["two"]
    ok, st, comb, nre = _wire(kzg, c, block, None, status=False)                 # drawn scalars, NULL for status
    assert (ok.tolist(), st, comb, nre) == (c.expect(block)[0], None) + c.expect(block)[2:], block


def test_what_the_mask_is_for(eng, kzg, cases):
    """the zero blob with 48 bytes of 0xff for both points: the decompression leaves all-zero records, which the equation takes for infinity,
    and the zero blob with C = pi = infinity holds -- the 0.21 call says 1 on those records, this call 0; the well-formed infinity stays valid"""
    _defaults(eng)
    c = cases["valid"]
    ff = next(j for j, e in EDGES.items() if e == "ff")
    zero = next(j for j, e in EDGES.items() if e == "zero")
    ok0 = kzg.verify_blob_batch(c.srs_g1, c.srs_g2, c.poly_bytes, c.k, b"".join(c.C), b"".join(c.pi), c.z_bytes, order=1, scalars=_pinned(M))[0]
    ok, st, comb, nre = _wire(kzg, c, 0, _pinned(M))
    assert (ok0[ff], ok[ff], st[ff]) == (1, 0, 0x12) and (ok0[zero], ok[zero], st[zero]) == (1, 1, 0)
    assert c.c48[zero] == c.p48[zero] == INF48 and (comb, nre) == (1, 0)         # the rejected items drag no block into the recheck
    nonc = next(j for j, e in EDGES.items() if isinstance(e, tuple) and e[0] == "noncanon")
    assert (ok0[nonc], ok[nonc], st[nonc]) == (1, 0, 0x40)                       # holds mod r, and is rejected


def test_one_batch_of_two_blobs_of_4096(eng, kzg):
    _defaults(eng)
    for spoil in ({}, {1: "f"}):
        c = WireCase(2, 12, SEED + 1, spoil=spoil)
        want = c.expect(0)
        assert want == ([1, 0 if spoil else 1], [0, 0], 0 if spoil else 1, 2 if spoil else 0)
        ok, st, comb, nre = _wire(kzg, c, 0, _pinned(2))
        assert (ok.tolist(), st.tolist(), comb, nre) == want


def test_no_blob(kzg, cases):
    c = cases["valid"]
    ok, st, comb, nre = kzg.verify_blob_batch_wire(c.srs_g1, c.srs_g2, b"", K, b"", b"")
    assert (ok.tolist(), st.tolist(), comb, nre) == ([], [], 0, 0)
    assert kzg.verify_blob_batch_wire_dev(0, 0, 0, K, 0, 0, 0, 0) == (0, 0)


@pytest.mark.parametrize("kind", ["valid", "two"])
def test_the_device_form(eng, kzg, cases, kind):
    import ctypes as C
    import torch
    _defaults(eng)
    c = cases[kind]
    want_ok, want_st, want_comb, want_nre = c.expect(8)
    scalars = _pinned(M)
    d_polys = _t(b"\xa5" * 4 + c.poly_bytes + b"\xa5" * 12)[4:4 + len(c.poly_bytes)]   # word-aligned only
    g, h, cm, pr = (_t(x) for x in (c.srs_g1, c.srs_g2, c.commitments48, c.proofs48))
    bufs = [g, h, d_polys, cm, pr]
    keep = [t.clone() for t in bufs]
    st = torch.cuda.Stream(device=g.device)
    for stream, sc, with_st in ((0, scalars, True), (st.cuda_stream, None, False)):
        d_ok = torch.full((M + 4,), 7, dtype=torch.uint8, device=g.device)
        d_st = torch.full((M + 4,), 7, dtype=torch.uint8, device=g.device)
        got = kzg.verify_blob_batch_wire_dev(g.data_ptr(), h.data_ptr(), d_polys.data_ptr(), K, cm.data_ptr(), pr.data_ptr(), M, d_ok.data_ptr(),
                                             d_status=d_st.data_ptr() if with_st else 0, scalars=sc, block=8, stream=stream)
        assert d_ok.cpu().numpy().tolist() == want_ok + [7] * 4 and got == (want_comb, want_nre), (kind, stream)
        assert d_st.cpu().numpy().tolist() == (want_st if with_st else [7] * M) + [7] * 4, (kind, stream)
    # the same call with the decompression on the main stream
    d_ok = torch.full((M,), 7, dtype=torch.uint8, device=g.device)
    d_st = torch.full((M,), 7, dtype=torch.uint8, device=g.device)
    comb, nre = C.c_int(0), C.c_size_t(0)
    eng._call("blsmi_debug_kzg_verify_blob_batch_wire_dev_serial", g.data_ptr(), h.data_ptr(), d_polys.data_ptr(), K, cm.data_ptr(), pr.data_ptr(), M,
              eng._scalars(scalars, M), 8, d_ok.data_ptr(), d_st.data_ptr(), C.byref(comb), C.byref(nre), st.cuda_stream)
    assert (d_ok.cpu().numpy().tolist(), d_st.cpu().numpy().tolist(), comb.value, nre.value) == (want_ok, want_st, want_comb, want_nre), kind
    for t, k in zip(bufs, keep):
        assert torch.equal(t, k), "the caller's device buffers are byte-identical afterwards"
