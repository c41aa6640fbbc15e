"""-m gpu: the launch layer (bls_amd/csrc/blsmi.hip: launch, kernels_of, tuple_blocks).  Every lane layout that has a row in the kernel
table -- row, quad, pair; the one-lane `single` kernels need BLSMI_LAYOUT=single at start-up, tests/test_gpu_startup_switches.py -- runs
Pairing, g2pubs / g1pubs Verify, FinalExponentiation and a pairing product at n = 1 and at n = 33: one more than the lane-pair kernels' 32
tuples a workgroup, so every layout ends in a partial workgroup (9 row workgroups, 3 quad, 2 pair; tuple 32 alone in the pair layout's
second).  Values and verdicts are the oracle's; the names of blsmi_last_profile are the lists below, which are the library's before the
launches went through one launcher: the tests, the launch-trace tools and bench.py's per-kernel breakdown key on those strings."""
import ctypes

import numpy as np
import pytest

from gpu_common import P, RC, rand_g1, rand_g2, sk_bytes

pytestmark = pytest.mark.gpu
N = 33
LAYOUTS = ("row", "quad", "pair")
SIZES = (1, N)

# Every list ends with the "(between)" from the call's last mark to the end of its context lease.
# Pairing: the Miller loop and the final exponentiation of the layout
PAIRING_NAMES = {l: ["k_miller1h_" + l, "k_final_exp_" + l, "(between)"] for l in LAYOUTS}
# Verify: the hash (a wave per map, the level program, the redo pass), the flag kernel's "(between)", the pair stage.  The row layout runs its
# signature side beside the hash, unmarked, and k_miller1m_row multiplies the other pair's loop onto it; with the quad threshold at 0 (pair)
# HashG1 is its one-lane kernel
VERIFY_NAMES = {
    ("g2pubs", "row"): ["k_swu_g1_waves", "k_lat:hashfin1", "k_hash_redo", "(between)", "k_miller1m_row", "k_final_exp_is_one_row", "(between)"],
    ("g2pubs", "quad"): ["k_swu_g1_two_lanes", "k_hash_g1_finish", "(between)", "k_miller2_quad", "k_final_exp_is_one_quad", "(between)"],
    ("g2pubs", "pair"): ["k_hash_g1", "(between)", "k_miller2_pair", "k_final_exp_is_one_pair", "(between)"],
    ("g1pubs", "row"): ["k_swu_g2_waves", "k_lat:hashfin2", "k_hash_redo", "(between)", "k_miller1m_row", "k_final_exp_is_one_row", "(between)"],
    ("g1pubs", "quad"): ["k_hash_g2_pair", "k_hash_redo", "(between)", "k_miller2_quad", "k_final_exp_is_one_quad", "(between)"],
    ("g1pubs", "pair"): ["k_hash_g2_pair", "k_hash_redo", "(between)", "k_miller2_pair", "k_final_exp_is_one_pair", "(between)"],
}
# FinalExponentiation launches unmarked in every layout
FINAL_EXP_NAMES = {"row": [], "single": []}
# the pairing product: one Miller value a pair (the skip kernel before it is unmarked), the segmented product, the final exponentiation of the two
# products (two values: the row layout's kernel under the row thresholds; beyond the latency path the quad layout's, the pair layout's with
# the quad threshold at 0), the comparison with one
PRODUCT_NAMES = {
    "row": ["k_miller1h_row", "k_fq12_seg_prod_row", "k_final_exp_row", "k_fq12_is_one_m384", "(between)"],
    "quad": ["k_miller1h_quad", "k_fq12_seg_prod_row", "k_final_exp_quad", "k_fq12_is_one_m384", "(between)"],
    "pair": ["k_miller1h_pair", "k_fq12_seg_prod_row", "k_final_exp_pair", "k_fq12_is_one_m384", "(between)"],
}


def force(eng, layout):
    """the layout of every call size, by the run-time setters (route.h: verify_layout); `single`: FinalExponentiation's one-lane kernel"""
    if layout == "row":
        eng.set_row_threshold(1, 8192)
    else:
        eng.set_latency_threshold(0)
        if layout == "pair":
            eng.set_quad_threshold(0)


@pytest.fixture(scope="module")
def eng():
    from bls_amd import engine
    engine.init(0)
    yield engine


@pytest.fixture
def layout_of(eng):
    yield lambda layout: force(eng, layout)
    eng.set_latency_threshold(8192); eng.set_quad_threshold(16384); eng.set_row_threshold(*eng.ROW_DEFAULT)


def names_of(eng, call):
    """call() with profiling on -> (its result, the names of blsmi_last_profile in order)"""
    lib = eng._lib()
    buf = ctypes.create_string_buffer(1 << 14)
    lib.blsmi_set_profiling(1); lib.blsmi_last_profile(buf, ctypes.c_size_t(len(buf)))
    try:
        out = call()
    finally:
        lib.blsmi_set_profiling(0)
    lib.blsmi_last_profile(buf, ctypes.c_size_t(len(buf)))
    return out, [item.split("=")[0] for item in buf.value.decode().split(";") if item]


@pytest.fixture(scope="module")
def points():
    xs = P.XORShift(1301)
    g1 = b"".join(rand_g1(xs) for _ in range(N)); g2 = b"".join(rand_g2(xs) for _ in range(N))
    return g1, g2, RC.pairing_batch(g1, g2, N)


@pytest.fixture(scope="module")
def signed():
    xs = P.XORShift(1302)
    sks = [sk_bytes(xs) for _ in range(N)]
    msgs = [b"launch table %d" % i for i in range(N)]
    return {name: (msgs, [o.priv_to_pub(k) for k in sks], [o.sign(m, k) for m, k in zip(msgs, sks)])
            for name, o in (("g2pubs", RC.g2pubs), ("g1pubs", RC.g1pubs))}


def test_one_pairing_through_the_kernel_table(eng, layout_of, points):
    """the smallest call: one tuple, the row layout's two kernels launched through the table's stored kernel pointers"""
    g1, g2, want = points
    layout_of("row")
    got, names = names_of(eng, lambda: eng.pairing_batch(g1[:96], g2[:192], 1))
    assert np.array_equal(got, want[:1])
    assert names == PAIRING_NAMES["row"], names


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_pairing(eng, layout_of, points, layout, n):
    g1, g2, want = points
    layout_of(layout)
    got, names = names_of(eng, lambda: eng.pairing_batch(g1[:96 * n], g2[:192 * n], n))
    assert np.array_equal(got, want[:n])
    assert names == PAIRING_NAMES[layout], names


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("group", ["g2pubs", "g1pubs"])
def test_verify(eng, layout_of, signed, group, layout, n):
    """all good; then one wrong signature (the first tuple's) at index n - 1: exactly that verdict is false, as the oracle's"""
    msgs, pks, sigs = signed[group]
    o = RC.g2pubs if group == "g2pubs" else RC.g1pubs
    fn = eng.g2pubs_verify_batch if group == "g2pubs" else eng.g1pubs_verify_batch
    layout_of(layout)
    (ok, _), names = names_of(eng, lambda: fn(msgs[:n], b"".join(pks[:n]), b"".join(sigs[:n])))
    assert list(ok) == [True] * n
    assert names == VERIFY_NAMES[group, layout], names
    wrong = sigs[:n - 1] + [sigs[0] if n > 1 else sigs[1]]
    assert o.verify(msgs[n - 1], pks[n - 1], wrong[n - 1]) is False
    (ok, _), names = names_of(eng, lambda: fn(msgs[:n], b"".join(pks[:n]), b"".join(wrong)))
    assert list(ok) == [True] * (n - 1) + [False]
    assert names == VERIFY_NAMES[group, layout], names


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("layout", ["row", "single"])
def test_final_exponentiation(eng, layout_of, points, layout, n):
    """the row layout's kernel out of the table, and beyond the latency path the one-lane k_final_exp"""
    g1, g2, want = points
    ml = np.stack([RC.miller_loop(g1[96 * i:96 * i + 96], g2[192 * i:192 * i + 192], 1) for i in range(n)])
    layout_of("row" if layout == "row" else "quad")                         # (the latency threshold at 0: FinalExponentiation has row, wave and single)
    got, names = names_of(eng, lambda: eng.final_exponentiation_batch(ml))
    assert np.array_equal(got, np.stack([RC.final_exponentiation(x)[1] for x in ml]))
    assert names == FINAL_EXP_NAMES[layout], names


@pytest.mark.parametrize("layout", LAYOUTS)
def test_pairing_product(eng, layout_of, points, layout):
    """segments [0, 1, 33]: one pair, and thirty-two"""
    g1, g2, want = points
    prods = [want[0], want[1]]
    for v in want[2:]:
        prods[1] = RC.fq12_mul(prods[1], v)
    layout_of(layout)
    (got, one), names = names_of(eng, lambda: eng.pairing_product_batch(g1, g2, [0, 1, N]))
    assert np.array_equal(got, np.stack(prods)) and list(one) == [0, 0]
    assert names == PRODUCT_NAMES[layout], names
