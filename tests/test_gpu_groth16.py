"""-m gpu: Groth16 batches with the public inputs folded in Fr (blsmi 0.19: blsmi_groth16_verify_batch[_jac|_dev|_jac_dev]).  The verdicts
against the oracle's four-pair FinalExponentiation(MillerLoop((A_j, B_j), (-alpha, beta), (-L_j, gamma), (-C_j, delta))) on the corpus of
tests/groth16_cases.py, `combined` saying whether the one equation held and `rechecked` how many items the per-item path saw, and the
kernels a call launches.  tests/test_groth16_cpu.py confirms the corpus and the folded block equation on the oracle alone."""
import pytest

from gpu_common import P, g1_to_jac, g2_to_jac, jac1, jac2
from groth16_cases import BAD_INPUT, BAD_TWO, M, Groth16Case, edges_for
from pprod_rlc_locate_common import rechecked_of
from test_gpu_pprod_rlc import _defaults, _pinned, _t
from test_gpu_pprod_rlc_segments import _segments

pytestmark = pytest.mark.gpu

BLOCKS = (0, 1, 8, 64)
# What an all-valid call of 37 proofs at block 8 launches, in order, recorded from the finished library: the 0.18 sums (weights, the delta
# cells' segmented sum, the singleton ladders), the fold, ONE full-width ladder launch over the 5 (nin + 2) gathered key points, the gamma
# cells' segmented sum, and the 0.18 stages.  No ladder launch but k_g1_mul_u64_idx has a count that scales with m, and that one is 64-bit.
VALID_NAMES = ["k_pprod_rlc_weights", "(between)", "k_g1_segsum_chunk_u64", "(between)", "k_g1_mul_u64_idx", "(between)", "k_fr_wsum_u64", "(between)",
               "k_lat:mul1", "(between)", "k_pprod_cell_route", "k_lat:miller1raw", "k_fq12_seg_prod_row", "k_lat:finalexp1", "k_fq12_is_one_m384", "(between)"]
FULL_WIDTH_LADDERS = ("k_g1_mul", "k_g1_mul_glv", "k_lat:mul1", "k_g1_msm", "k_g1_segsum_chunk_u64_pair")


@pytest.fixture(scope="module")
def eng():
    from bls_amd import engine
    engine.init(0)
    yield engine
    _defaults(engine)


@pytest.fixture(scope="module")
def cases():
    """every batch with the oracle's verdicts, computed once"""
    out = {}
    for nin in (3, 1):
        out[nin, "valid"] = Groth16Case(M, nin, 19)
        out[nin, "input"] = Groth16Case(M, nin, 19, spoil=BAD_INPUT)
        out[nin, "two"] = Groth16Case(M, nin, 19, spoil=BAD_TWO)
        out[nin, "edges"] = Groth16Case(M, nin, 19, **edges_for(nin))
    out[0, "valid"] = Groth16Case(M, 0, 19)
    out[0, "two"] = Groth16Case(M, 0, 19, spoil=BAD_TWO)
    out[3, "B"] = Groth16Case(M, 3, 19, spoil={30: "B"})
    out = {k: (c, c.verdicts()) for k, c in out.items()}
    for (nin, kind), (c, v) in out.items():
        bad = {"input": BAD_INPUT, "two": BAD_TWO, "B": {30: "B"}}.get(kind, {})
        assert v == [0 if j in bad else 1 for j in range(M)], (nin, kind)
    return out


def _host(eng, c, block, scalars):
    return eng.groth16_verify_batch(c.vk_g1, c.vk_g2, c.proof_g1, c.proof_g2, c.input_bytes if c.nin else None, c.nin, scalars, block)


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("nin", [3, 1])
def test_verdicts_combined_and_rechecked(eng, cases, nin, block):
    _defaults(eng)
    for kind, bad in (("valid", ()), ("input", tuple(BAD_INPUT)), ("two", tuple(BAD_TWO)), ("edges", ())):
        c, v = cases[nin, kind]
        ok, comb, nre = _host(eng, c, block, _pinned(M))
        assert ok.tolist() == v, (nin, kind, block)                              # item by item, the oracle's
        assert comb == (0 if bad else 1), (nin, kind, block)
        assert nre == rechecked_of(M, block, bad), (nin, kind, block)
    assert rechecked_of(M, block, tuple(BAD_TWO)) == {0: 37, 1: 2, 8: 16, 64: 37}[block]


def test_drawn_scalars(eng, cases):
    _defaults(eng)
    for nin in (3, 1):
        c, v = cases[nin, "valid"]
        assert (lambda r: (r[0].tolist(), r[1], r[2]))(_host(eng, c, 8, None)) == (v, 1, 0)
        c, v = cases[nin, "input"]
        assert (lambda r: (r[0].tolist(), r[1], r[2]))(_host(eng, c, 8, None)) == (v, 0, 8)


def test_no_public_input_and_a_replaced_b(eng, cases):
    _defaults(eng)
    for block in BLOCKS:
        for kind, bad in (("valid", ()), ("two", tuple(BAD_TWO))):
            c, v = cases[0, kind]
            ok, comb, nre = _host(eng, c, block, _pinned(M))
            assert (ok.tolist(), comb, nre) == (v, 0 if bad else 1, rechecked_of(M, block, bad)), (kind, block)
    c, v = cases[3, "B"]
    ok, comb, nre = _host(eng, c, 8, _pinned(M))
    assert (ok.tolist(), comb, nre) == (v, 0, rechecked_of(M, 8, (30,)))
    ok, comb, nre = eng.groth16_verify_batch(c.vk_g1, c.vk_g2, b"", b"", b"", 3)
    assert (ok.tolist(), comb, nre) == ([], 0, 0)


def test_an_all_zero_key_entry_drops_its_pairs(eng, cases):
    """gamma all-zero: the (L_j, gamma) pairs contribute 1, in the combined path and in the recheck alike -- the proofs built for the real
    gamma then fail, item by item, as the four-pair product without that pair does"""
    _defaults(eng)
    c, _ = cases[3, "valid"]
    vk2 = c.beta_g2 + bytes(192) + c.delta_g2
    from groth16_cases import fe_of_pairs, is_one
    want = [int(is_one(fe_of_pairs([p for i, p in enumerate(c.four_pairs(j)) if i != 2]))) for j in range(4)]
    assert want == [0] * 4
    ok, comb, nre = eng.groth16_verify_batch(c.vk_g1, vk2, c.proof_g1[:4 * 192], c.proof_g2[:4 * 192], c.input_bytes[:4 * 96], 3, _pinned(4), 2)
    assert (ok.tolist(), comb, nre) == (want, 0, 4)


def _jac_case(c, seed):
    xs = P.XORShift(seed)
    j1 = lambda rec: b"".join(g1_to_jac(None, 0) if rec[k:k + 96] == bytes(96) else jac1(xs, rec[k:k + 96]) for k in range(0, len(rec), 96))     # noqa: E731
    j2 = lambda rec: b"".join(g2_to_jac(None) if rec[k:k + 192] == bytes(192) else jac2(xs, rec[k:k + 192]) for k in range(0, len(rec), 192))   # noqa: E731
    return j1(c.vk_g1), j2(c.vk_g2), j1(c.proof_g1), j2(c.proof_g2)


@pytest.mark.parametrize("kind", ["valid", "two", "edges"])
def test_every_form(eng, cases, kind):
    import torch
    _defaults(eng)
    c, v = cases[3, kind]
    bad = tuple(BAD_TWO) if kind == "two" else ()
    want = (0 if bad else 1, rechecked_of(M, 8, bad))
    scalars = _pinned(M)
    jk1, jk2, jp1, jp2 = _jac_case(c, 5)
    ok, comb, nre = eng.groth16_verify_batch_jac(jk1, jk2, jp1, jp2, c.input_bytes, 3, scalars, 8)
    assert (ok.tolist(), (comb, nre)) == (v, want)
    d_in = _t(c.input_bytes)
    st = torch.cuda.Stream(device=d_in.device)
    for jac in (False, True):
        bufs = [_t(x) for x in ((jk1, jk2, jp1, jp2) if jac else (c.vk_g1, c.vk_g2, c.proof_g1, c.proof_g2))] + [d_in]
        keep = [t.clone() for t in bufs]
        f = eng.groth16_verify_batch_jac_dev if jac else eng.groth16_verify_batch_dev
        for stream, sc in ((0, scalars), (st.cuda_stream, None)):
            d_ok = torch.full((M,), 7, dtype=torch.uint8, device=d_in.device)
            got = f(bufs[0].data_ptr(), bufs[1].data_ptr(), 3, bufs[2].data_ptr(), bufs[3].data_ptr(), d_in.data_ptr(), M, d_ok.data_ptr(), scalars=sc, block=8, stream=stream)
            assert d_ok.cpu().numpy().tolist() == v and got == want, (jac, stream)
        for t, k in zip(bufs, keep):
            assert torch.equal(t, k), "the caller's device buffers are byte-identical afterwards"


def test_dev_form_over_records_that_are_only_word_aligned(eng, cases):
    import torch
    _defaults(eng)
    c, v = cases[3, "two"]
    shifted = []
    for x in (c.vk_g1, c.proof_g1, c.input_bytes):
        buf = _t(b"\xa5" * 4 + x + b"\xa5" * 12)
        shifted.append((buf, buf[4:4 + len(x)]))
        assert shifted[-1][1].data_ptr() % 16 == 4
    d_vk2, d_p2 = _t(c.vk_g2), _t(c.proof_g2)
    keep = [b.clone() for b, _ in shifted]
    d_ok = torch.full((M,), 7, dtype=torch.uint8, device=d_vk2.device)
    got = eng.groth16_verify_batch_dev(shifted[0][1].data_ptr(), d_vk2.data_ptr(), 3, shifted[1][1].data_ptr(), d_p2.data_ptr(), shifted[2][1].data_ptr(), M, d_ok.data_ptr(),
                                       scalars=_pinned(M), block=8)
    assert d_ok.cpu().numpy().tolist() == v and got == (0, 16)
    for (b, _), k in zip(shifted, keep):
        assert torch.equal(b, k)


def test_the_kernels_a_call_launches(eng, cases):
    """all valid: the fold is there and no full-width ladder launch scales with m -- the one ladder launch is over the B (nin + 2) gathered
    key points, whatever m (the same list at m = 37 and m = 16, both at block 8: 5 and 2 blocks); a failing call runs the recheck stages once"""
    _defaults(eng)
    c, v = cases[3, "valid"]
    (ok, comb, nre), names = _segments(eng, lambda: _host(eng, c, 8, _pinned(M)))
    assert (ok.tolist(), comb, nre) == (v, 1, 0)
    assert names == VALID_NAMES, names
    assert "k_fr_wsum_u64" in names
    assert [n for n in names if any(n == w or n.endswith(w) for w in FULL_WIDTH_LADDERS)] == ["k_lat:mul1"]
    assert names.index("k_fr_wsum_u64") < names.index("k_lat:mul1") < names.index("k_pprod_cell_route")
    (ok, comb, nre), fewer = _segments(eng, lambda: eng.groth16_verify_batch(c.vk_g1, c.vk_g2, c.proof_g1[:16 * 192], c.proof_g2[:16 * 192], c.input_bytes[:16 * 96], 3, _pinned(16), 8))
    assert (ok.tolist(), comb, nre) == ([1] * 16, 1, 0) and fewer == names
    c, v = cases[3, "two"]
    (ok, comb, nre), names = _segments(eng, lambda: _host(eng, c, 8, _pinned(M)))
    assert (ok.tolist(), comb, nre) == (v, 0, 16)
    assert names[:len(VALID_NAMES) - 1] == VALID_NAMES[:-1], names
    for once in ("k_gather_records16", "k_groth16_recheck_pairs", "k_scatter_bytes"):
        assert names.count(once) == 1, (once, names)
    assert names.count("k_fr_wsum_u64") == 2                                     # the blocks' fold, and the rechecked items' inputs mod r
