"""-m gpu: KZG cell batches (blsmi 0.22: blsmi_kzg_verify_cell_batch[_jac|_dev|_jac_dev]): the cells are interpolated over their cosets on the
device, the coefficients folded per block, and the rest is the pairing side of blsmi_kzg_verify_batch.  Verdicts, `combined`, `rechecked` and
`flags` against the big-integer expectation of tests/cell_cases.py (tau is known: a cell holds exactly when
c - I(tau) + h^n q = q tau^n mod r), each way of spoiling one item, the edge items, n = 1 against blsmi_kzg_verify_batch itself, one batch
shaped as EIP-7594 shapes its cells, and the four forms."""
import pytest

from cell_cases import EDGES, L, M, ORDER, SEED, SPOILS, CellCase, cell_shifts
from fr_eval_cases import R
from gpu_common import P, g1_to_jac, g2_to_jac, jac1, jac2
from kzg_cases import INF, KzgCase
from kzg_cases import EDGES as KZG_EDGES, M as KZG_M, SEED as KZG_SEED, SPOILS as KZG_SPOILS
from pprod_rlc_locate_common import rechecked_of
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
    """every batch with the big-integer verdicts, computed once"""
    out = {"valid": CellCase(M, L, ORDER, SEED, edge=EDGES)}
    for kind, spoil in SPOILS.items():
        out[kind] = CellCase(M, L, ORDER, SEED, spoil=spoil, edge=EDGES)
    out = {k: (c, c.verdicts()) for k, c in out.items()}
    for kind, (c, v) in out.items():
        assert v == [0 if j in SPOILS.get(kind, {}) else 1 for j in range(M)], kind   # each spoils its items only
        assert c.pi[8] == INF and not any(c.coeffs[9]) and [c.flags[j] for j in (2, 3, 4, 6, 10)] == [1, 2, 3, 1, 1], kind
    return out


def _cell(kzg, c, block, scalars, **kw):
    return kzg.verify_cell_batch(c.srs_g1, c.srs_g2, c.vals_bytes, c.l, c.shift_bytes, c.commitments, c.proofs, order=c.order, scalars=scalars, block=block, **kw)


@pytest.mark.parametrize("block", BLOCKS)
def test_verdicts_combined_rechecked_and_flags(eng, kzg, cases, block):
    _defaults(eng)
    for kind, (c, v) in cases.items():
        bad = tuple(SPOILS.get(kind, ()))
        ok, fl, comb, nre = _cell(kzg, c, block, _pinned(M))
        assert (ok.tolist(), comb, nre) == (v, 0 if bad else 1, rechecked_of(M, block, bad)), (kind, block)   # the big-integer expectation
        assert fl.tolist() == c.flags, (kind, block)                             # ok = 1 whatever the flags say
    c, v = cases["two"]
    ok, fl, comb, nre = _cell(kzg, c, block, None, flags=False)                  # drawn scalars, NULL for flags
    assert (ok.tolist(), fl, comb, nre) == (v, None, 0, rechecked_of(M, block, tuple(SPOILS["two"])))


def test_one_value_per_cell_is_the_opening_of_a_point(eng, kzg):
    """n = 1: the coset is the point h, the interpolant the value, [tau^n] H = tau H -- the call returns exactly what blsmi_kzg_verify_batch
    returns on (C, pi, z = h, y = the value) under the same scalars, on that call's own corpus with its edges and spoils"""
    _defaults(eng)
    for kind, spoil in [("valid", {})] + sorted(KZG_SPOILS.items()):
        c = KzgCase(KZG_M, KZG_SEED, spoil=spoil, edge=KZG_EDGES)
        for block in (0, 8):
            want = kzg.verify_batch(c.srs_g1, c.srs_g2, c.commitments, c.proofs, c.z_bytes, c.y_bytes, _pinned(KZG_M), block)
            ok, fl, comb, nre = kzg.verify_cell_batch(c.srs_g1, c.srs_g2, c.y_bytes, 0, c.z_bytes, c.commitments, c.proofs, order=kind == "valid", scalars=_pinned(KZG_M), block=block)
            assert (ok.tolist(), comb, nre) == (want[0].tolist(), want[1], want[2]), (kind, block)
            assert ok.tolist() == [0 if j in spoil else 1 for j in range(KZG_M)], (kind, block)
            assert fl.tolist() == [(1 if z >= R or y >= R else 0) | (2 if z % R == 0 else 0) for z, y in zip(c.z, c.y)], (kind, block)


def test_cells_of_an_extended_blob(eng, kzg):
    """n = 64, order 1, the shifts of kzg.cell_shifts(7, 6): five cells each of two polynomials, valid and with one value spoiled"""
    _defaults(eng)
    hs = cell_shifts(7, 6)
    picks = [0, 1, 2, 77, 127, 5, 64, 100, 126, 3]
    assert [int.from_bytes(bytes(r), "big") for r in kzg.cell_shifts(7, 6)] == hs
    edge = {j: ("poly_of", 0 if j < 5 else 5) for j in (1, 2, 3, 4, 6, 7, 8, 9)}
    for spoil in ({}, {7: "v"}):
        c = CellCase(10, 6, 1, SEED + 1, spoil=spoil, edge=edge, shifts=[hs[k] for k in picks])
        v = c.verdicts()
        assert v == [0 if j in spoil else 1 for j in range(10)] and len({bytes(x) for x in c.C}) == 2 and c.h == [hs[k] for k in picks]
        ok, fl, comb, nre = _cell(kzg, c, 0, _pinned(10))
        assert (ok.tolist(), fl.tolist(), comb, nre) == (v, [0] * 10, 0 if spoil else 1, 10 if spoil else 0)


def test_no_cell(kzg, cases):
    c, _ = cases["valid"]
    ok, fl, comb, nre = kzg.verify_cell_batch(c.srs_g1, c.srs_g2, b"", L, b"", b"", b"")
    assert (ok.tolist(), fl.tolist(), comb, nre) == ([], [], 0, 0)
    assert kzg.verify_cell_batch_dev(0, 0, 0, L, 1, 0, 0, 0, 0, 0) == (0, 0)


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
    ok, fl, comb, nre = kzg.verify_cell_batch_jac(jg, jh, c.vals_bytes, L, c.shift_bytes, jc, jp, order=ORDER, scalars=scalars, block=8)
    assert (ok.tolist(), fl.tolist(), (comb, nre)) == (v, c.flags, want)
    d_vals = _t(b"\xa5" * 4 + c.vals_bytes + b"\xa5" * 12)[4:4 + len(c.vals_bytes)]   # word-aligned only: the interpolation reads it byte by byte
    d_h = _t(c.shift_bytes)
    st = torch.cuda.Stream(device=d_h.device)
    for jac in (False, True):
        g, h, cm, pr = (_t(x) for x in ((jg, jh, jc, jp) if jac else (c.srs_g1, c.srs_g2, c.commitments, c.proofs)))
        bufs = [g, h, d_vals, d_h, cm, pr]
        keep = [t.clone() for t in bufs]
        f = kzg.verify_cell_batch_jac_dev if jac else kzg.verify_cell_batch_dev
        for stream, sc, with_fl in ((0, scalars, True), (st.cuda_stream, None, False)):
            d_ok = torch.full((M,), 7, dtype=torch.uint8, device=d_h.device)
            d_fl = torch.full((M,), 7, dtype=torch.uint8, device=d_h.device)
            got = f(g.data_ptr(), h.data_ptr(), d_vals.data_ptr(), L, ORDER, d_h.data_ptr(), cm.data_ptr(), pr.data_ptr(), M, d_ok.data_ptr(),
                    d_flags=d_fl.data_ptr() if with_fl else 0, scalars=sc, block=8, stream=stream)
            assert d_ok.cpu().numpy().tolist() == v and got == want, (jac, stream)
            assert d_fl.cpu().numpy().tolist() == (c.flags if with_fl else [7] * M), (jac, stream)
        for t, k in zip(bufs, keep):
            assert torch.equal(t, k), "the caller's device buffers are byte-identical afterwards"
