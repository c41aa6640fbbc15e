"""-m gpu: KZG blob batches (blsmi 0.21: blsmi_kzg_verify_blob_batch[_jac|_dev|_jac_dev]): the blob is evaluated on the device and the rest
is blsmi_kzg_verify_batch.  Verdicts, `combined` and `rechecked` against kzg.verify_batch given the model's y AND against the big-integer
expectation of tests/fr_eval_cases.py (tau is known: an item holds exactly when c - y + z q = q tau mod r), each way of spoiling one
item, the edge items, and the four forms."""
import pytest

from fr_eval_cases import BlobCase, domain
from gpu_common import P, g1_to_jac, g2_to_jac, jac1, jac2
from kzg_cases import INF, M
from pprod_rlc_locate_common import rechecked_of
from test_gpu_pprod_rlc import _defaults, _pinned, _t

pytestmark = pytest.mark.gpu

K, ORDER, SEED = 4, 1, 21
BLOCKS = (0, 1, 8, 64)
# item 3: z is a root; item 9: a value written as v + r; item 10: a constant blob, pi at infinity
EDGES = {3: ("root", 6), 9: ("noncanon", 2), 10: "const"}
SPOILS = {"f": {5: "f"}, "z": {14: "z"}, "C": {30: "C"}, "pi": {33: "pi"}, "root": {3: "f"}, "two": {7: "C", 21: "f"}}


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
    """every batch with the big-integer verdicts, computed once"""
    out = {"valid": BlobCase(M, K, ORDER, SEED, edge=EDGES)}
    for kind, spoil in SPOILS.items():
        out[kind] = BlobCase(M, K, ORDER, SEED, spoil=spoil, edge=EDGES)
    out = {k: (c, c.verdicts()) for k, c in out.items()}
    for kind, (c, v) in out.items():
        assert v == [0 if j in SPOILS.get(kind, {}) else 1 for j in range(M)], kind   # each spoils its items only
        assert c.noncanon == [j == 9 for j in range(M)] and c.pi[10] == INF and c.z[3] % (1 << 256) == domain(K, ORDER)[6], kind
    valid = out["valid"][0]
    for kind in ("f", "root"):                                                   # only the blob moved: the points of the spoiled item are the valid batch's
        c, j = out[kind][0], next(iter(SPOILS[kind]))
        assert (c.C[j], c.pi[j], c.z[j]) == (valid.C[j], valid.pi[j], valid.z[j]) and c.polys[j] != valid.polys[j] and c.y[j] != valid.y[j], kind
    return out


def _blob(kzg, c, block, scalars, **kw):
    return kzg.verify_blob_batch(c.srs_g1, c.srs_g2, c.poly_bytes, c.k, c.commitments, c.proofs, c.z_bytes, order=c.order, scalars=scalars, block=block, **kw)


@pytest.mark.parametrize("block", BLOCKS)
def test_verdicts_combined_and_rechecked(eng, kzg, cases, block):
    _defaults(eng)
    for kind, (c, v) in cases.items():
        bad = tuple(SPOILS.get(kind, ()))
        ok, nc, comb, nre = _blob(kzg, c, block, _pinned(M))
        ok0, comb0, nre0 = kzg.verify_batch(c.srs_g1, c.srs_g2, c.commitments, c.proofs, c.z_bytes, c.y_bytes, _pinned(M), block)   # the model's y
        assert (ok.tolist(), comb, nre) == (ok0.tolist(), comb0, nre0), (kind, block)
        assert (ok.tolist(), comb, nre) == (v, 0 if bad else 1, rechecked_of(M, block, bad)), (kind, block)   # the big-integer expectation
        assert nc.tolist() == c.noncanon, (kind, block)                          # ok = 1 and noncanon = 1 at item 9
    c, v = cases["two"]
    ok, nc, comb, nre = _blob(kzg, c, block, None, noncanon=False)               # drawn scalars, NULL for noncanon
    assert (ok.tolist(), nc, comb, nre) == (v, None, 0, rechecked_of(M, block, tuple(SPOILS["two"])))


def test_one_batch_of_two_blobs_of_4096(eng, kzg):
    _defaults(eng)
    for spoil in ({}, {1: "f"}):
        c = BlobCase(2, 12, 1, SEED + 1, spoil=spoil, edge={0: ("noncanon", 4095)})
        v = c.verdicts()
        assert v == [1, 0 if spoil else 1]
        ok, nc, comb, nre = _blob(kzg, c, 0, _pinned(2))
        assert (ok.tolist(), nc.tolist(), comb, nre) == (v, [True, False], 0 if spoil else 1, 2 if spoil else 0)
        assert kzg.verify_batch(c.srs_g1, c.srs_g2, c.commitments, c.proofs, c.z_bytes, c.y_bytes, _pinned(2), 0)[0].tolist() == v


def test_no_blob(kzg, cases):
    c, _ = cases["valid"]
    ok, nc, comb, nre = kzg.verify_blob_batch(c.srs_g1, c.srs_g2, b"", K, b"", b"", b"")
    assert (ok.tolist(), nc.tolist(), comb, nre) == ([], [], 0, 0)
    assert kzg.verify_blob_batch_dev(0, 0, 0, K, 1, 0, 0, 0, 0, 0) == (0, 0)


def _jac_case(c, seed):
    xs = P.XORShift(seed)
    j1 = lambda rec: b"".join(g1_to_jac(None, 0) if rec[k:k + 96] == INF else jac1(xs, rec[k:k + 96]) for k in range(0, len(rec), 96))       # noqa: E731
    j2 = lambda rec: b"".join(g2_to_jac(None) if rec[k:k + 192] == bytes(192) else jac2(xs, rec[k:k + 192]) for k in range(0, len(rec), 192))   # noqa: E731
    return j1(c.srs_g1), j2(c.srs_g2), j1(c.commitments), j1(c.proofs)


@pytest.mark.parametrize("kind", ["valid", "two"])
def test_every_form(eng, kzg, cases, kind):
    import torch
    _defaults(eng)
    c, v = cases[kind]
    bad = tuple(SPOILS.get(kind, ()))
    want = (0 if bad else 1, rechecked_of(M, 8, bad))
    scalars = _pinned(M)
    jg, jh, jc, jp = _jac_case(c, 5)
    ok, nc, comb, nre = kzg.verify_blob_batch_jac(jg, jh, c.poly_bytes, K, jc, jp, c.z_bytes, order=ORDER, scalars=scalars, block=8)
    assert (ok.tolist(), nc.tolist(), (comb, nre)) == (v, c.noncanon, want)
    d_polys = _t(b"\xa5" * 4 + c.poly_bytes + b"\xa5" * 12)[4:4 + len(c.poly_bytes)]   # word-aligned only: the evaluation reads it byte by byte
    d_z = _t(c.z_bytes)
    st = torch.cuda.Stream(device=d_z.device)
    for jac in (False, True):
        g, h, cm, pr = (_t(x) for x in ((jg, jh, jc, jp) if jac else (c.srs_g1, c.srs_g2, c.commitments, c.proofs)))
        bufs = [g, h, d_polys, cm, pr, d_z]
        keep = [t.clone() for t in bufs]
        f = kzg.verify_blob_batch_jac_dev if jac else kzg.verify_blob_batch_dev
        for stream, sc, with_nc in ((0, scalars, True), (st.cuda_stream, None, False)):
            d_ok = torch.full((M,), 7, dtype=torch.uint8, device=d_z.device)
            d_nc = torch.full((M,), 7, dtype=torch.uint8, device=d_z.device)
            got = f(g.data_ptr(), h.data_ptr(), d_polys.data_ptr(), K, ORDER, cm.data_ptr(), pr.data_ptr(), d_z.data_ptr(), M, d_ok.data_ptr(),
                    d_noncanon=d_nc.data_ptr() if with_nc else 0, scalars=sc, block=8, stream=stream)
            assert d_ok.cpu().numpy().tolist() == v and got == want, (jac, stream)
            assert d_nc.cpu().numpy().tolist() == ([int(x) for x in c.noncanon] if with_nc else [7] * M), (jac, stream)
        for t, k in zip(bufs, keep):
            assert torch.equal(t, k), "the caller's device buffers are byte-identical afterwards"
