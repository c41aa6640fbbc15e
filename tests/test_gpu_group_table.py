"""-m gpu: the host routines of the group operations (bls_amd/csrc/blsmi.hip: GroupKernels, group_kernels) -- scalar multiplication,
PrivToPub, sums, MSM, segmented sums, compression, decompression and ToAffine -- for G1 and G2 at n = 1 and n = 67: a full one-lane
workgroup of 64 plus a ragged one, and a ragged third workgroup of the lane-pair kernels' 32 items.  Every path the run-time setters
select: the level programs (defaults), the lane kernels (latency threshold 0), the plain ladder (any_point).  Values are the oracle's; the
names of blsmi_last_profile are the lists below, recorded from the library as it stood before the group routines took their kernels from one
table row per group: the tests, the launch-trace tools and bench.py's per-kernel breakdown key on those strings.  The bucket-method MSM
is covered by tests/test_gpu_startup_switches.py (msm-bucket-min-1*) and tests/test_gpu_group_edges.py."""
import numpy as np
import pytest

from gpu_common import P, RC, g1_to_jac, g2_to_jac, jac1, jac2, rand_g1, rand_g2, sk_bytes
from test_gpu_launch_table import names_of

pytestmark = pytest.mark.gpu
N = 67
SIZES = (1, N)
GROUPS = (1, 2)
PB = {1: 96, 2: 192}
B = "(between)"          # from a call's last mark to the end of its context lease, and between marked kernels

# case -> group -> the names of blsmi_last_profile; every case gives the same list at each of its sizes
NAMES = {
    # scalar multiplication of given points: the level program, the endomorphism ladder, the plain ladder (G2: the lane-pair kernels)
    "mul/lat": {1: ["k_lat:mul1", B], 2: ["k_lat:mul2", B]},
    "mul/glv": {1: ["k_g1_mul_glv", B], 2: ["k_g2_mul_glv_pair", B]},
    "mul/plain": {1: ["k_g1_mul", B], 2: ["k_g2_mul_pair", B]},
    # PrivToPub over the generator's fixed-base table: a wave per scalar, a lane per scalar; the _jac forms add an unmarked conversion
    "gen/wave": {1: ["k_g1_mul_fixed_wave", B], 2: ["k_g2_mul_fixed_wave", B]},
    "gen/lane": {1: ["k_g1_mul_fixed", B], 2: ["k_g2_mul_fixed", B]},
    # sums: the level programs open one segment for the whole tree; the tree kernels: level 0, the levels above, the last record.
    # In-memory points become wire records first on the latency path and are added as they are (k_g?_sum0_jac, named k_g?_sum0) beyond it
    "sum/lat": {1: ["k_lat:sum", B], 2: ["k_lat:sum", B]},
    "sum/tree": {1: ["k_g1_sum0", "k_g1_sum", "k_g1_sum_final", B], 2: ["k_g2_sum0", "k_g2_sum", "k_g2_sum_final", B]},
    "sum_jac/lat": {1: ["k_g1_jac_to_affine", B, "k_lat:sum", B], 2: ["k_g2_jac_to_affine", B, "k_lat:sum", B]},
    "sum_jac/tree": {1: ["k_g1_sum0", "k_g1_sum", "k_g1_sum_final", B], 2: ["k_g2_sum0", "k_g2_sum", "k_g2_sum_final", B]},
    # MSM below the bucket method: the multiples (which close their segment), then their sum
    "msm/lat": {1: ["k_lat:mul1", B, "k_lat:sum", B], 2: ["k_lat:mul2", B, "k_lat:sum", B]},
    "msm/glv": {1: ["k_g1_mul_glv", B, "k_g1_sum0", "k_g1_sum", "k_g1_sum_final", B], 2: ["k_g2_mul_glv_pair", B, "k_g2_sum0", "k_g2_sum", "k_g2_sum_final", B]},
    "msm/plain": {1: ["k_g1_mul", B, "k_g1_sum0", "k_g1_sum", "k_g1_sum_final", B], 2: ["k_g2_mul_pair", B, "k_g2_sum0", "k_g2_sum", "k_g2_sum_final", B]},
    "msm/plain-lat": {1: ["k_g1_mul", B, "k_lat:sum", B], 2: ["k_g2_mul_pair", B, "k_lat:sum", B]},
    # segmented sums launch unmarked; the weighted form marks its ladder pass
    "segsum": {1: [], 2: []},
    "segsum_jac": {1: [], 2: []},
    "segsum_u64": {1: ["k_g1_segsum_chunk_u64", B], 2: ["k_g2_segsum_chunk_u64", B]},
    # decompression: a wave per point without the subgroup check; with it the same and the level program of the check; beyond the latency path
    # the lane kernel, which checks by itself
    "decompress/waves": {1: ["k_g1_decompress_waves", B], 2: ["k_g2_decompress_waves", B]},
    "decompress/lat": {1: ["k_g1_decompress_waves", "k_lat:subgrp1", B], 2: ["k_g2_decompress_waves", "k_lat:subgrp2", B]},
    "decompress/lane": {1: ["k_g1_decompress", B], 2: ["k_g2_decompress", B]},
    "compress": {1: [], 2: []},
    "jac_to_affine": {1: ["k_g1_jac_to_affine", B], 2: ["k_g2_jac_to_affine", B]},
}


def expect(case, group, n, names):
    assert names == NAMES[case][group], (case, group, n, names)


@pytest.fixture(scope="module")
def eng():
    from bls_amd import engine
    engine.init(0)
    yield engine


@pytest.fixture
def lanes(eng):
    """-> a function that takes the latency path away (threshold 0); the default comes back after the test"""
    yield lambda: eng.set_latency_threshold(0)
    eng.set_latency_threshold(8192)


class Data:
    """N seeded points of each group, scalars, and everything the oracle says about them, computed once"""

    def __init__(self):
        xs = P.XORShift(1401)
        self.pts = {1: [rand_g1(xs) for _ in range(N)], 2: [rand_g2(xs) for _ in range(N)]}
        self.ks = [sk_bytes(xs) for _ in range(N)]
        self.u64 = [P.rand_int(xs, 1 << 64) for _ in range(N)]
        self.jac = {1: [jac1(xs, w) for w in self.pts[1]], 2: [jac2(xs, w) for w in self.pts[2]]}
        mul = {1: RC.g1_mul, 2: RC.g2_mul}
        gen = {1: RC.g1_generator(), 2: RC.g2_generator()}
        self.mul = {g: [mul[g](p, k) for p, k in zip(self.pts[g], self.ks)] for g in GROUPS}
        self.gen = {g: [mul[g](gen[g], k) for k in self.ks] for g in GROUPS}
        self.mul_u64 = {g: [mul[g](p, k.to_bytes(32, "big")) for p, k in zip(self.pts[g], self.u64)] for g in GROUPS}
        self.compressed = {1: [RC.g1_compress(w) for w in self.pts[1]], 2: [RC.g2_compress(w) for w in self.pts[2]]}

    @staticmethod
    def sum(group, pts, flags=None):
        """the oracle's sum of a list of wire points -> bytes | None"""
        return (RC.g1_sum if group == 1 else RC.g2_sum)(b"".join(pts), len(pts), flags)


@pytest.fixture(scope="module")
def data():
    return Data()


def rows(out, inf):
    """(n, pb) records + infinity flags -> the oracle's form: bytes | None per point"""
    return [None if f else bytes(r) for r, f in zip(out, inf)]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("path", ["lat", "glv", "plain"])
@pytest.mark.parametrize("group", GROUPS)
def test_mul(eng, lanes, data, group, path, n):
    fn = eng.g1_mul_batch if group == 1 else eng.g2_mul_batch
    if path != "lat":
        lanes()
    (out, inf), names = names_of(eng, lambda: fn(b"".join(data.pts[group][:n]), b"".join(data.ks[:n]), n, any_point=path == "plain"))
    assert rows(out, inf) == data.mul[group][:n]
    expect("mul/" + path, group, n, names)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("jac", [False, True], ids=["affine", "jac"])
@pytest.mark.parametrize("path", ["wave", "lane"])
@pytest.mark.parametrize("group", GROUPS)
def test_mul_generator(eng, lanes, data, group, path, jac, n):
    if path == "lane":
        lanes()
    ks = b"".join(data.ks[:n])
    if jac:
        fn = eng.g1_mul_generator_batch_jac if group == 1 else eng.g2_mul_generator_batch_jac
        recs, names = names_of(eng, lambda: fn(ks, n))
        got = RC.jac_to_affine_bytes_batch(group, np.ascontiguousarray(recs).reshape(-1).view(np.uint64), n).reshape(n, PB[group])
        assert [bytes(r) for r in got] == data.gen[group][:n]
    else:
        fn = eng.g1_mul_generator_batch if group == 1 else eng.g2_mul_generator_batch
        (out, inf), names = names_of(eng, lambda: fn(ks, n))
        assert rows(out, inf) == data.gen[group][:n]
    expect("gen/" + path, group, n, names)


@pytest.mark.parametrize("n", (1, 2, N))
@pytest.mark.parametrize("path", ["lat", "tree"])
@pytest.mark.parametrize("group", GROUPS)
def test_sum(eng, lanes, data, group, path, n):
    """from n = 2 on, point n // 2 is flagged at infinity"""
    fn = eng.g1_sum if group == 1 else eng.g2_sum
    flags = None if n == 1 else bytes(1 if i == n // 2 else 0 for i in range(n))
    if path == "tree":
        lanes()
    got, names = names_of(eng, lambda: fn(b"".join(data.pts[group][:n]), n, flags))
    assert got == data.sum(group, data.pts[group][:n], flags)
    expect("sum/" + path, group, n, names)


@pytest.mark.parametrize("n", (1, 2, N))
@pytest.mark.parametrize("path", ["lat", "tree"])
@pytest.mark.parametrize("group", GROUPS)
def test_sum_jac(eng, lanes, data, group, path, n):
    """in-memory points in, the in-memory sum out; from n = 2 on, point n // 2 has z = 0"""
    fn = eng.g1_sum_jac if group == 1 else eng.g2_sum_jac
    to_jac = g1_to_jac if group == 1 else g2_to_jac
    flags = None if n == 1 else bytes(1 if i == n // 2 else 0 for i in range(n))
    recs = [to_jac(w, 0 if group == 1 else (0, 0)) if flags and flags[i] else j for i, (w, j) in enumerate(zip(data.pts[group][:n], data.jac[group][:n]))]
    if path == "tree":
        lanes()
    (s, inf), names = names_of(eng, lambda: fn(b"".join(recs), n))
    want = data.sum(group, data.pts[group][:n], flags)
    assert inf == (want is None)
    assert bytes(RC.jac_to_affine_bytes_batch(group, np.frombuffer(s, dtype=np.uint64), 1)) == want
    expect("sum_jac/" + path, group, n, names)


@pytest.mark.parametrize("path", ["lat", "glv", "plain", "plain-lat"])
@pytest.mark.parametrize("group", GROUPS)
def test_msm(eng, lanes, data, group, path):
    """67 points: below the bucket method, so the multiples and their sum -- level programs, lane kernels, the plain ladder with either sum"""
    fn = eng.g1_msm if group == 1 else eng.g2_msm
    if path in ("glv", "plain"):
        lanes()
    got, names = names_of(eng, lambda: fn(b"".join(data.pts[group]), b"".join(data.ks), N, any_point=path.startswith("plain")))
    assert got == data.sum(group, data.mul[group])
    expect("msm/" + path, group, N, names)


@pytest.mark.parametrize("form", ["segsum", "segsum_jac", "segsum_u64"])
@pytest.mark.parametrize("group", GROUPS)
def test_sum_segmented(eng, data, group, form):
    """segments [0, 1, 67]: one point, and sixty-six"""
    seg = [0, 1, N]
    pts = data.pts[group]
    if form == "segsum":
        fn = eng.g1_sum_segmented if group == 1 else eng.g2_sum_segmented
        (out, inf), names = names_of(eng, lambda: fn(b"".join(pts), N, None, seg))
    elif form == "segsum_jac":
        fn = eng.g1_sum_segmented_jac if group == 1 else eng.g2_sum_segmented_jac
        (out, inf), names = names_of(eng, lambda: fn(b"".join(data.jac[group]), N, None, seg))
    else:
        fn = eng.g1_sum_segmented_u64 if group == 1 else eng.g2_sum_segmented_u64
        pts = data.mul_u64[group]
        (out, inf), names = names_of(eng, lambda: fn(b"".join(data.pts[group]), N, data.u64, None, seg))
    assert list(inf) == [0, 0]
    assert out == pts[0] + data.sum(group, pts[1:])
    expect(form, group, N, names)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("path", ["waves", "lat", "lane"])
@pytest.mark.parametrize("group", GROUPS)
def test_decompress(eng, lanes, data, group, path, n):
    fn = eng.g1_decompress_batch if group == 1 else eng.g2_decompress_batch
    if path == "lane":
        lanes()
    (out, inf, err), names = names_of(eng, lambda: fn(b"".join(data.compressed[group][:n]), n, path != "waves"))
    assert not err.any() and not inf.any()
    assert [bytes(r) for r in out] == data.pts[group][:n]
    expect("decompress/" + path, group, n, names)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("group", GROUPS)
def test_compress(eng, data, group, n):
    fn = eng.g1_compress_batch if group == 1 else eng.g2_compress_batch
    out, names = names_of(eng, lambda: fn(b"".join(data.pts[group][:n]), n))
    assert [bytes(r) for r in out] == data.compressed[group][:n]
    expect("compress", group, n, names)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("group", GROUPS)
def test_jac_to_affine(eng, data, group, n):
    fn = eng.g1_jac_to_affine_batch if group == 1 else eng.g2_jac_to_affine_batch
    recs = b"".join(data.jac[group][:n])
    (out, inf), names = names_of(eng, lambda: fn(recs, n))
    assert not inf.any()
    assert out == bytes(RC.jac_to_affine_bytes_batch(group, np.frombuffer(recs, dtype=np.uint64), n)) == b"".join(data.pts[group][:n])
    expect("jac_to_affine", group, n, names)
