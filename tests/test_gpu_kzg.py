"""-m gpu: KZG batches with the values folded in Fr (blsmi 0.20: blsmi_kzg_verify_batch[_jac|_dev|_jac_dev]).  The verdicts against the
oracle's two-pair FinalExponentiation(MillerLoop((C_j + z_j pi_j - y_j G, H), (pi_j, -tau H))) on the corpus of tests/kzg_cases.py,
`combined` saying whether the one equation held and `rechecked` how many items the per-item path saw, and the kernels a call launches.
tests/test_kzg_cpu.py confirms the corpus and the folded block equation on the oracle alone."""
import pytest

from gpu_common import P, g1_to_jac, g2_to_jac, jac1, jac2
from kzg_cases import BAD_TWO, EDGES, INF, M, SEED, SPOILS, KzgCase
from pprod_rlc_locate_common import rechecked_of
from test_gpu_groth16 import FULL_WIDTH_LADDERS
from test_gpu_pprod_rlc import _defaults, _pinned, _t
from test_gpu_pprod_rlc_segments import _segments

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
    """every batch with the oracle's verdicts, computed once"""
    out = {"valid": KzgCase(M, SEED), "edges": KzgCase(M, SEED, edge=EDGES)}
    for kind, spoil in SPOILS.items():
        out[kind] = KzgCase(M, SEED, spoil=spoil)
    out = {k: (c, c.verdicts()) for k, c in out.items()}
    for kind, (c, v) in out.items():
        assert v == [0 if j in SPOILS.get(kind, {}) else 1 for j in range(M)], kind
    return out


def _host(kzg, c, block, scalars, m=None):
    m = c.m if m is None else m
    return kzg.verify_batch(c.srs_g1, c.srs_g2, c.commitments[:96 * m], c.proofs[:96 * m], c.z_bytes[:32 * m], c.y_bytes[:32 * m], scalars, block)


def _flat(r):
    return r[0].tolist(), r[1], r[2]


@pytest.mark.parametrize("block", BLOCKS)
def test_verdicts_combined_and_rechecked(eng, kzg, cases, block):
    _defaults(eng)
    for kind in ("valid", "y", "z", "C", "pi", "two", "edges"):
        c, v = cases[kind]
        bad = tuple(SPOILS.get(kind, ()))
        ok, comb, nre = _host(kzg, c, block, _pinned(M))
        assert ok.tolist() == v, (kind, block)                                   # item by item, the oracle's
        assert comb == (0 if bad else 1), (kind, block)
        assert nre == rechecked_of(M, block, bad), (kind, block)
    assert rechecked_of(M, block, tuple(BAD_TWO)) == {0: 37, 1: 2, 8: 16, 64: 37}[block]


@pytest.mark.parametrize("block", BLOCKS)
def test_drawn_scalars(eng, kzg, cases, block):
    _defaults(eng)
    for kind in ("valid", "edges", "y", "two"):
        c, v = cases[kind]
        bad = tuple(SPOILS.get(kind, ()))
        assert _flat(_host(kzg, c, block, None)) == (v, 0 if bad else 1, rechecked_of(M, block, bad)), (kind, block)
    assert _flat(kzg.verify_batch(cases["valid"][0].srs_g1, cases["valid"][0].srs_g2, b"", b"", b"", b"")) == ([], 0, 0)


def test_an_all_zero_tau_h_drops_its_pairs(eng, kzg, cases):
    """tau H all-zero: the (pi_j, -tau H) pairs contribute 1, in the combined path and in the recheck alike -- the verdicts are those of the
    one-pair product (P_j, H): one exactly where P_j = [q_j tau] G is at infinity"""
    _defaults(eng)
    c, _ = cases["edges"]
    n = 14
    want = c.verdicts((c.H, bytes(192)))[:n]
    assert want == [1 if j == 10 else 0 for j in range(n)]
    for block in (0, 1, 4):
        ok, comb, nre = kzg.verify_batch(c.srs_g1, c.H + bytes(192), c.commitments[:96 * n], c.proofs[:96 * n], c.z_bytes[:32 * n], c.y_bytes[:32 * n], _pinned(n), block)
        assert (ok.tolist(), comb, nre) == (want, 0, n - 1 if block == 1 else n), block
    # H all-zero as well: nothing is left of any item
    ok, comb, nre = kzg.verify_batch(c.srs_g1, bytes(384), c.commitments[:96 * n], c.proofs[:96 * n], c.z_bytes[:32 * n], c.y_bytes[:32 * n], _pinned(n), 4)
    assert (ok.tolist(), comb, nre) == ([1] * n, 1, 0)


def _jac_case(c, seed):
    xs = P.XORShift(seed)
    j1 = lambda rec: b"".join(g1_to_jac(None, 0) if rec[k:k + 96] == INF else jac1(xs, rec[k:k + 96]) for k in range(0, len(rec), 96))       # noqa: E731
    j2 = lambda rec: b"".join(g2_to_jac(None) if rec[k:k + 192] == bytes(192) else jac2(xs, rec[k:k + 192]) for k in range(0, len(rec), 192))   # noqa: E731
    return j1(c.srs_g1), j2(c.srs_g2), j1(c.commitments), j1(c.proofs)


@pytest.mark.parametrize("kind", ["valid", "two", "edges"])
def test_every_form(eng, kzg, cases, kind):
    import torch
    _defaults(eng)
    c, v = cases[kind]
    bad = tuple(BAD_TWO) if kind == "two" else ()
    want = (0 if bad else 1, rechecked_of(M, 8, bad))
    scalars = _pinned(M)
    jg, jh, jc, jp = _jac_case(c, 5)
    ok, comb, nre = kzg.verify_batch_jac(jg, jh, jc, jp, c.z_bytes, c.y_bytes, scalars, 8)
    assert (ok.tolist(), (comb, nre)) == (v, want)
    d_z, d_y = _t(c.z_bytes), _t(c.y_bytes)
    st = torch.cuda.Stream(device=d_z.device)
    for jac in (False, True):
        bufs = [_t(x) for x in ((jg, jh, jc, jp) if jac else (c.srs_g1, c.srs_g2, c.commitments, c.proofs))] + [d_z, d_y]
        keep = [t.clone() for t in bufs]
        f = kzg.verify_batch_jac_dev if jac else kzg.verify_batch_dev
        for stream, sc in ((0, scalars), (st.cuda_stream, None)):
            d_ok = torch.full((M,), 7, dtype=torch.uint8, device=d_z.device)
            got = f(*(t.data_ptr() for t in bufs), M, d_ok.data_ptr(), scalars=sc, block=8, stream=stream)
            assert d_ok.cpu().numpy().tolist() == v and got == want, (jac, stream)
        for t, k in zip(bufs, keep):
            assert torch.equal(t, k), "the caller's device buffers are byte-identical afterwards"


def test_dev_form_over_records_that_are_only_word_aligned(eng, kzg, cases):
    import torch
    _defaults(eng)
    c, v = cases["two"]
    shifted = []
    for x in (c.srs_g1, c.srs_g2, c.commitments, c.proofs, c.z_bytes, c.y_bytes):
        buf = _t(b"\xa5" * 4 + x + b"\xa5" * 12)
        shifted.append((buf, buf[4:4 + len(x)]))
        assert shifted[-1][1].data_ptr() % 16 == 4
    keep = [b.clone() for b, _ in shifted]
    d_ok = torch.full((M,), 7, dtype=torch.uint8, device=keep[0].device)
    got = kzg.verify_batch_dev(*(s.data_ptr() for _, s in shifted), M, d_ok.data_ptr(), scalars=_pinned(M), block=8)
    assert d_ok.cpu().numpy().tolist() == v and got == (0, 16)
    for (b, _), k in zip(shifted, keep):
        assert torch.equal(b, k)


def test_three_hundred_items_at_the_automatic_block(eng, kzg):
    """block 0 at m = 300: five blocks of 64, the last one of 44 with the one spoiled item"""
    _defaults(eng)
    m, bad = 300, {290: "y"}
    c = KzgCase(m, SEED + 1, spoil=bad)
    v = c.verdicts()
    assert v == [0 if j in bad else 1 for j in range(m)]
    assert _flat(_host(kzg, c, 0, _pinned(m))) == (v, 0, 44) and rechecked_of(m, 0, tuple(bad)) == 44
    assert _flat(_host(kzg, c, 0, None, m=256)) == ([1] * 256, 1, 0)             # the first four blocks alone hold


def _ladders(names):
    return [n for n in names if any(n == w or n.endswith(w) for w in FULL_WIDTH_LADDERS)]


def test_the_kernels_a_call_launches(eng, kzg, cases):
    """all valid: the lift once, the fold once, and no full-width ladder launch but the one over the B copies of -G, whatever m (the same list
    at m = 37 and m = 16, both at block 8: 5 and 2 blocks); a failing call runs the recheck stages once and the lift still once"""
    _defaults(eng)
    c, v = cases["valid"]
    (ok, comb, nre), names = _segments(eng, lambda: _host(kzg, c, 8, _pinned(M)))
    assert (ok.tolist(), comb, nre) == (v, 1, 0)
    assert names.count("k_g1_mul_add_glv") == 1 and names.count("k_fr_wsum_u64") == 1, names
    assert len(_ladders(names)) == 1, names                                      # s_b (-G): one launch over B = 5 multiplicands
    lad = _ladders(names)[0]
    assert names.index("k_g1_mul_add_glv") < names.index("k_pprod_rlc_weights") < names.index("k_fr_wsum_u64") < names.index(lad) < names.index("k_pprod_cell_route"), names
    assert "k_kzg_recheck_pairs" not in names and "k_scatter_bytes" not in names
    (ok, comb, nre), fewer = _segments(eng, lambda: _host(kzg, c, 8, _pinned(16), m=16))
    assert (ok.tolist(), comb, nre) == ([1] * 16, 1, 0) and fewer == names
    c, v = cases["two"]
    (ok, comb, nre), failing = _segments(eng, lambda: _host(kzg, c, 8, _pinned(M)))
    assert (ok.tolist(), comb, nre) == (v, 0, 16)
    assert failing[:len(names) - 1] == names[:-1], failing                       # the holding path's stages first, as they were
    for once in ("k_g1_mul_add_glv", "k_gather_records16", "k_kzg_recheck_pairs", "k_scatter_bytes"):
        assert failing.count(once) == 1, (once, failing)
    assert failing.count("k_fr_wsum_u64") == 2                                   # the blocks' fold, and the rechecked items' values mod r
    assert len(_ladders(failing)) == 2, failing                                  # s_b (-G) and the rechecked items' y_j (-G)
