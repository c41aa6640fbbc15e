"""-m gpu: every message length 0 .. 200 on every route of HashG1 and HashG2 (hash.go:306-331, 391-411).

All routes begin with sha256_msg (hash.cuh) over 0x01 || message, read bytewise from the packed message buffer; k_hash.hip, k_hash_pair.hip
and the other kernel files each compile their own copy.  With the prefix, messages of 54, 118 and 182 bytes are the last that fit their
one, two and three blocks with the padding (55, 119 and 183 open the next block).  The 201 messages here have the lengths 0, 1, ..., 200 and
lie back to back, so message i starts at offset i (i - 1) / 2 and every start offset modulo 16 occurs.  Each route -- forced by the
run-time options, confirmed by the kernel names of blsmi_last_profile -- must give the oracle's bytes for all 201; a route that needs more
messages gets the list three times over.  Routes that only a start-up variable selects belong to tests/test_gpu_startup_switches.py."""
import numpy as np
import pytest

from gpu_common import RC
from test_gpu_miller_variants import names_of

pytestmark = pytest.mark.gpu

MSGS = [bytes((7 * length + 13 * j + 1) & 0xff for j in range(length)) for length in range(201)]
assert {sum(range(i)) % 16 for i in range(201)} == set(range(16))          # the start offsets of the packed messages
DEFAULTS = {"swu_row_max": 4096, "hash_row_min": 2048, "hash_row_max": 4096, "hash_quad_min": 4097, "hash_quad_max": 16384,
            "hash_oct_min": 2048, "hash_oct_max": 7168, "hash_g1_quad_min": 1280, "hash_g1_quad_max": 32768}

# route -> (latency threshold, options, repeats of the list, kernel names the profile must hold)
G1_ROUTES = {
    "waves+hashfin1": (8192, {}, 1, ("k_swu_g1_waves", "k_lat:hashfin1")),
    "rows+hashfin1": (8192, {}, 3, ("k_swu_g1_rows", "k_lat:hashfin1")),
    "two_lanes+hashfin1": (8192, {"swu_row_max": 0}, 3, ("k_swu_g1_two_lanes", "k_lat:hashfin1")),
    "two_lanes+finish": (0, {"hash_g1_quad_max": 0}, 1, ("k_swu_g1_two_lanes", "k_hash_g1_finish")),
    "two_lanes+finish_quad": (8192, {"hash_g1_quad_min": 1}, 1, ("k_swu_g1_two_lanes", "k_hash_g1_finish_quad")),
}
G2_ROUTES = {
    "waves+hashfin2": (8192, {}, 1, ("k_swu_g2_waves", "k_lat:hashfin2")),
    "rows+hashfin2": (8192, {}, 3, ("k_swu_g2_rows", "k_lat:hashfin2")),
    "two_lanes+hashfin2": (8192, {"swu_row_max": 0}, 3, ("k_swu_g2_two_lanes", "k_lat:hashfin2")),
    "pair": (0, {}, 1, ("k_hash_g2_pair",)),
    "front+clear_row": (8192, {"hash_oct_max": 0, "hash_row_min": 1}, 1, ("k_hash_g2_front", "k_clear_h2_row")),
    "front+clear_oct": (8192, {"hash_oct_min": 1}, 1, ("k_hash_g2_front", "k_clear_h2_oct")),
    "front+clear_quad": (8192, {"hash_oct_max": 0, "hash_row_max": 0, "hash_quad_min": 1}, 1, ("k_hash_g2_front", "k_clear_h2_quad")),
}


@pytest.fixture(scope="module")
def eng():
    from bls_amd import engine
    engine.init(0)
    engine.set_latency_threshold(8192)
    yield engine
    engine.set_latency_threshold(8192)


@pytest.fixture(scope="module")
def want():
    """the oracle's hash points of the 201 messages, computed once"""
    return {1: [RC.hash_g1(m) for m in MSGS], 2: [RC.hash_g2(m) for m in MSGS]}


def _route(eng, fn, route, want):
    threshold, options, repeats, kernels = route
    try:
        eng.set_latency_threshold(threshold)
        for k, v in options.items():
            eng.set_option(k, v)
        out, names = names_of(eng, lambda: fn(MSGS * repeats))
    finally:
        eng.set_latency_threshold(8192)
        for k in options:
            eng.set_option(k, DEFAULTS[k])
    assert all(k in names for k in kernels), names
    assert not any(k.startswith(("k_swu_", "k_hash_g", "k_clear_h2", "k_lat:hashfin")) and k not in kernels for k in names), names
    for j in range(len(MSGS) * repeats):
        assert out[j].tobytes() == want[j % 201], ("record", j, "length", j % 201)


@pytest.mark.parametrize("route", sorted(G1_ROUTES))
def test_hash_g1_of_every_length(eng, want, route):
    _route(eng, eng.hash_g1_batch, G1_ROUTES[route], want[1])


@pytest.mark.parametrize("route", sorted(G2_ROUTES))
def test_hash_g2_of_every_length(eng, want, route):
    _route(eng, eng.hash_g2_batch, G2_ROUTES[route], want[2])


@pytest.mark.parametrize("kind", [0, 1], ids=["hash_g1", "hash_g2"])
def test_one_lane_hash_of_every_length(eng, want, kind):
    """hash_g1 / hash_g2 (hash.cuh), one lane per message from the digest to the point, through blsmi_debug_hash_redo with every good flag 0
    (the entry point launches k_hash_g1_redo / k_hash_g2_redo unconditionally and leaves no profile mark)"""
    hb = 96 if kind == 0 else 192
    out = eng.debug_hash_redo(kind, MSGS, np.zeros(201, dtype=np.uint8), np.full((201, hb), 0xAA, dtype=np.uint8))
    for j in range(201):
        assert out[j].tobytes() == want[kind + 1][j], ("length", j)
