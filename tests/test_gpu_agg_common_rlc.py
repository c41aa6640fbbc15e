"""-m gpu: randomised verification of many committee aggregates in one call (blsmi 0.16: blsmi_g?pubs_verify_aggregate_common*_batch_rlc
[_jac|_dev]) and the lane-pair weighted pass 1 under it (k_g2_segsum_chunk_u64_pair, through blsmi_debug_g2_sum_segmented_u64_pair).
Item j is VerifyAggregateCommon(sig_j, committee j of the registry, table[msg_idx[j]]).  Expectations come from the oracle, as
tests/test_gpu_agg_common_batch.py takes them: verify_aggregate_common per item (valid aggregates are signed with the committee's summed
secret key), sums of multiples for the kernel; the equation itself is tests/test_agg_common_rlc_cpu.py: committee_holds.

Run as a program (`python tests/test_gpu_agg_common_rlc.py workload.npz`) this file is the worker of the BLSMI_LAYOUT=single test: a fresh
process that reads its inputs from the file and prints verdicts and kernel names as one JSON line."""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

import numpy as np
import pytest

from gpu_common import P, RC, g1_to_jac, g2_to_jac, jac1, jac2
from test_gpu_launch_table import names_of
from test_gpu_rlc_grouped import weighted_cases  # noqa: F401  (the corpus of the weighted segmented sums, as a fixture of this module too)

pytestmark = pytest.mark.gpu
KINDS = ("g2pubs", "g1pubs", "domain")
DOMAIN = bytes(range(1, 9))
EDGE = [1, 1 << 63, (1 << 64) - 1, 2]
NPK = 48
SIZES = [1, 2, 3, 8, 9, 65, 130, 1, 2, 3, 8, 9]                            # m = 12 committees
PER_ITEM = ("k_miller2", "k_final_exp_is_one", "k_lat:verify")             # the pair stage of a verify batch, in any layout
CHILD_LIMIT_S = 120


@pytest.fixture(scope="module")
def eng():
    from bls_amd import engine
    engine.init(0)
    yield engine
    engine.set_option("segsum_chunk", 0)


def _neg(p, group):
    if group == 1:
        return p[:48] + ((P.Q - int.from_bytes(p[48:], "big")) % P.Q).to_bytes(48, "big")
    return p[:96] + b"".join(((P.Q - int.from_bytes(p[o:o + 48], "big")) % P.Q).to_bytes(48, "big") for o in (96, 144))


# ---- 1. the lane-pair weighted pass 1, bit for bit -------------------------------------------------------------------------------------
def _check_sums(got, ginf, want, winf, what):
    assert ginf.tolist() == winf, what
    for j in range(len(winf)):
        assert got[192 * j:192 * (j + 1)] == want[192 * j:192 * (j + 1)], (what, j)


def test_lane_pair_pass1_bit_for_bit(eng, weighted_cases):  # noqa: F811
    """the corpus of tests/test_gpu_rlc_grouped.py (empty, one point, one index twice, P and -P, in_inf, a zero scalar, scalars 1, 2, 2^63,
    2^64 - 1, lengths 65 and 130: 209 chunks, six full workgroups of 32 pairs and a ragged one) through the lane-pair kernel; at
    segsum_chunk 1 the folds add two partials at a time (130 -> 65 -> 33)"""
    pts, in_inf, r, idx, off, want, winf = weighted_cases[2]
    try:
        for K in (0, 1, 2, 1024):
            eng.set_option("segsum_chunk", K)
            (got, ginf), names = names_of(eng, lambda: eng.debug_g2_sum_segmented_u64_pair(pts, 48, r, idx, off, in_inf))
            _check_sums(got, ginf, want, winf, ("pair", K))
            assert names[0] == "k_g2_segsum_chunk_u64_pair", names
            (got, ginf), names = names_of(eng, lambda: eng.g2_sum_segmented_u64(pts, 48, r, idx, off, in_inf))
            _check_sums(got, ginf, want, winf, ("one lane", K))
            assert names[0] == "k_g2_segsum_chunk_u64", names                    # the entry point of 0.11 keeps the one-lane kernel
    finally:
        eng.set_option("segsum_chunk", 0)
    # an odd number of chunks, by positions: 3 points in one segment, then 1, then 31 (35 chunks: one full workgroup and three pairs)
    seg = [0, 3, 4, 35]
    got, ginf = eng.debug_g2_sum_segmented_u64_pair(pts, 48, r, None, seg)
    assert ginf.tolist() == [0, 0, 0]
    for j in range(3):
        parts = [RC.g2_mul(pts[192 * i:192 * (i + 1)], r[i].to_bytes(32, "big")) for i in range(seg[j], seg[j + 1]) if r[i]]
        assert got[192 * j:192 * (j + 1)] == RC.g2_sum(b"".join(parts), len(parts)), j


# ---- 2. the call ------------------------------------------------------------------------------------------------------------------------
class Items:
    """m committee aggregates over one registry of 48 keys (key 47 = -key 0), every one valid by construction (signed with the summed secret key)"""

    def __init__(self, eng, kind, sizes, d, seed):
        self.kind, self.d = kind, d
        self.pkg = RC.g2pubs if kind == "g2pubs" else RC.g1pubs
        self.kg, self.sg = (2, 1) if kind == "g2pubs" else (1, 2)
        rng = np.random.default_rng(seed)
        sk = rng.integers(0, 256, size=(NPK, 32), dtype=np.uint8)
        sk[:, 0] &= 0x3f
        self.ski = [int.from_bytes(sk[i].tobytes(), "big") for i in range(NPK)]
        self.ski[NPK - 1] = (-self.ski[0]) % P.R_ORDER
        skb = b"".join(x.to_bytes(32, "big") for x in self.ski)
        keys, _ = (eng.g1_mul_generator_batch if self.kg == 1 else eng.g2_mul_generator_batch)(skb, NPK)
        self.registry = [bytes(keys[i]) for i in range(NPK)]
        assert self.registry[NPK - 1] == _neg(self.registry[0], self.kg)
        m = len(sizes)
        self.comm = [[int(x) for x in rng.integers(1, NPK - 1, size=L)] for L in sizes]   # (with repeats from 65 keys on; never key 0 or its negative)
        for c in self.comm:
            if len(c) >= 3:
                c[2] = c[0]                                                      # one index twice
        if kind == "domain":
            self.table = [hashlib.sha256(b"committee-rlc %d %d" % (seed, g)).digest() for g in range(d)]
        else:
            self.table = [b"attestation data %d/%d" % (seed, g) + b"z" * (g % 3) for g in range(d)]
        self.msg_idx = [j % d for j in range(m)]
        self.sigs = self.sign(eng, self.comm, self.msg_idx)
        self.m = m

    def sign(self, eng, comm, msg_idx):
        ssum = b"".join((sum(self.ski[i] for i in c) % P.R_ORDER or 1).to_bytes(32, "big") for c in comm)
        msgs = [self.table[g] for g in msg_idx]
        if self.kind == "g2pubs":
            sigs, _ = eng.g2pubs_sign_batch(msgs, ssum)
        elif self.kind == "g1pubs":
            sigs, _ = eng.g1pubs_sign_batch(msgs, ssum)
        else:
            sigs, _ = eng.g1pubs_sign_with_domain_batch(msgs, DOMAIN, ssum)
        return [bytes(s) for s in sigs]

    def oracle(self, comm, msg_idx, sigs, j):
        pks = [self.registry[i] for i in comm[j] if i < NPK]
        if not any(sigs[j]) or any(i >= NPK for i in comm[j]):
            return False
        if self.kind == "domain":
            return bool(pks) and self.pkg.verify_aggregate_common_with_domain(sigs[j], pks, self.table[msg_idx[j]], DOMAIN)
        return self.pkg.verify_aggregate_common(sigs[j], pks, self.table[msg_idx[j]])


def _flat(comm):
    return np.array([i for c in comm for i in c], dtype=np.uint32), np.cumsum([0] + [len(c) for c in comm]).astype(np.uint64)


def _t(b):
    import torch
    a = np.frombuffer(bytes(b), dtype=np.uint8).copy() if not isinstance(b, np.ndarray) else np.ascontiguousarray(b).view(np.uint8).reshape(-1).copy()
    if a.size == 0:
        a = np.zeros(8, dtype=np.uint8)
    return torch.from_numpy(a).to(torch.device("cuda", 0))


def _jac(it, sigs):
    xs = P.XORShift(77)
    keys = b"".join((jac1 if it.kg == 1 else jac2)(xs, p) for p in it.registry)
    sj = b"".join((jac1 if it.sg == 1 else jac2)(xs, s) if any(s) else (g1_to_jac if it.sg == 1 else g2_to_jac)(None) for s in sigs)
    return keys, sj


def run_rlc(eng, it, form, comm, msg_idx, sigs, scalars=None):
    """-> (ok list, combined) of the randomised call in one of its three forms"""
    idx, off = _flat(comm)
    k = it.kind
    if form == "dev":
        import torch
        if k == "domain":
            d_m, d_mo = _t(b"".join(it.table)), _t(DOMAIN)
        else:
            d_m, d_mo = _t(b"".join(it.table)), _t(np.cumsum([0] + [len(x) for x in it.table]).astype(np.uint64))
        d_pk, d_x, d_off, d_s, d_mi = _t(b"".join(it.registry)), _t(idx), _t(off), _t(b"".join(sigs)), _t(np.asarray(msg_idx, np.uint32))
        d_ok = torch.full((len(comm),), 7, dtype=torch.uint8, device=torch.device("cuda", 0))
        comb = eng.verify_aggregate_common_batch_rlc_dev("g2pubs" if k == "g2pubs" else "g1pubs", d_m.data_ptr(), d_mo.data_ptr(), it.d, d_mi.data_ptr(), d_pk.data_ptr(),
                                                         NPK, d_x.data_ptr(), d_off.data_ptr(), d_s.data_ptr(), d_ok.data_ptr(), len(comm), scalars, domain=(k == "domain"))
        return [bool(x) for x in d_ok.cpu().numpy()], comb
    if form == "jac":
        keys, sg = _jac(it, sigs)
        sfx = "_jac"
    else:
        keys, sg, sfx = b"".join(it.registry), b"".join(sigs), ""
    if k == "domain":
        ok, bm, comb = getattr(eng, "g1pubs_verify_aggregate_common_with_domain_batch_rlc" + sfx)(it.table, DOMAIN, msg_idx, keys, NPK, idx, off, sg, scalars)
    else:
        ok, bm, comb = getattr(eng, "%s_verify_aggregate_common_batch_rlc%s" % (k, sfx))(it.table, msg_idx, keys, NPK, idx, off, sg, scalars)
    assert np.array_equal(np.packbits(np.asarray(ok, np.uint8), bitorder="little")[:len(bm)], bm)
    return [bool(x) for x in ok], comb


def run_09(eng, it, comm, msg_idx, sigs, dev=False):
    """the verdicts of blsmi_g?pubs_verify_aggregate_common*_batch (blsmi 0.9) for the same inputs, messages expanded"""
    idx, off = _flat(comm)
    msgs = [it.table[g] for g in msg_idx]
    k = it.kind
    if dev:
        import torch
        d_m = _t(b"".join(msgs))
        d_mo = _t(DOMAIN) if k == "domain" else _t(np.cumsum([0] + [len(x) for x in msgs]).astype(np.uint64))
        d_pk, d_x, d_off, d_s = _t(b"".join(it.registry)), _t(idx), _t(off), _t(b"".join(sigs))
        d_ok = torch.zeros(len(comm), dtype=torch.uint8, device=torch.device("cuda", 0))
        eng.verify_aggregate_common_batch_dev("g2pubs" if k == "g2pubs" else "g1pubs", d_m.data_ptr(), d_mo.data_ptr(), d_pk.data_ptr(), NPK, d_x.data_ptr(), d_off.data_ptr(),
                                              d_s.data_ptr(), d_ok.data_ptr(), len(comm), domain=(k == "domain"))
        return [bool(x) for x in d_ok.cpu().numpy()]
    keys, sg = b"".join(it.registry), b"".join(sigs)
    if k == "domain":
        ok, _ = eng.g1pubs_verify_aggregate_common_with_domain_batch(b"".join(msgs), DOMAIN, keys, NPK, idx, off, sg)
    else:
        ok, _ = getattr(eng, "%s_verify_aggregate_common_batch" % k)(msgs, keys, NPK, idx, off, sg)
    return [bool(x) for x in ok]


@pytest.fixture(scope="module")
def items(eng):
    """per kind: m = 12 items over the 48-key registry, d = 3, committee sizes {1, 2, 3, 8, 9, 65, 130}; all valid by the oracle"""
    out = {}
    for n, kind in enumerate(KINDS):
        it = Items(eng, kind, SIZES, 3, seed=900 + n)
        assert all(it.oracle(it.comm, it.msg_idx, it.sigs, j) for j in range(it.m)), kind
        out[kind] = it
    return out


SCALARS = EDGE + [0x9e3779b97f4a7c15, 3, 0xdeadbeefcafef00d, 1 << 32, 0x0123456789abcdef, 5, (1 << 64) - 59, 0x8000000000000001]


@pytest.mark.parametrize("kind", KINDS)
def test_all_valid_one_equation(eng, items, kind):
    it = items[kind]
    for form in ("host", "jac", "dev"):
        for sc in (SCALARS, None):
            (ok, comb), names = names_of(eng, lambda: run_rlc(eng, it, form, it.comm, it.msg_idx, it.sigs, sc))
            assert comb == 1 and ok == [True] * it.m, (kind, form, sc is None)
            # the segmented sum with its pass 1 (G2: the lane-pair ladder -- the key side for g2pubs, the signature side for g1pubs), the d' = 3
            # Miller loops as one launch of wave programs, and no per-item pair stage
            assert "k_g2_segsum_chunk_u64_pair" in names and "k_g2_segsum_chunk_u64" not in names, (kind, form, names)
            assert "k_g1_segsum_chunk_u64" in names, (kind, form, names)         # (the other side's sum: G1 has one lane per ladder)
            assert names.count("k_lat:miller1raw") == 1, (kind, form, names)
            assert not [x for x in names if x.startswith(PER_ITEM)], (kind, form, names)


@pytest.mark.parametrize("kind", KINDS)
def test_each_corruption_alone(eng, items, kind):
    """combined is 0, the verdict vector is the oracle's and the 0.9 call's, every other item stays 1"""
    it = items[kind]
    m = it.m

    def check(what, comm, msg_idx, sigs, bad, forms=("host", "jac", "dev"), dev09=False):
        want = [True] * m
        for j in bad:
            want[j] = it.oracle(comm, msg_idx, sigs, j)                          # (the other items' inputs are the fixture's: valid by the oracle)
            assert want[j] is False, (kind, what, j)
        assert run_09(eng, it, comm, msg_idx, sigs, dev=dev09) == want, (kind, what, "0.9")
        for form in forms:
            (ok, comb), names = names_of(eng, lambda: run_rlc(eng, it, form, comm, msg_idx, sigs, SCALARS))
            assert comb == 0 and ok == want, (kind, what, form, ok)
            assert [x for x in names if x.startswith(PER_ITEM)], (kind, what, form, names)   # the m Verify()s ran
        assert run_rlc(eng, it, forms[0], comm, msg_idx, sigs, None) == (want, 0), (kind, what, "drawn scalars")

    s = list(it.sigs); s[5] = it.sigs[8]                                         # a wrong signature (items 5 and 8 share message 2)
    check("wrong signature", it.comm, it.msg_idx, s, [5])
    c = [list(x) for x in it.comm]; c[6][77] = (c[6][77] % (NPK - 2)) + 1        # a committee member replaced (by its neighbour in the registry)
    assert c[6][77] != it.comm[6][77]
    check("member replaced", c, it.msg_idx, it.sigs, [6])
    mi = list(it.msg_idx); mi[4] = (mi[4] + 1) % it.d                            # an item under the wrong message
    check("wrong message", it.comm, mi, it.sigs, [4])
    c = [list(x) for x in it.comm]; c[3] = []                                    # an empty committee
    check("empty committee", c, it.msg_idx, it.sigs, [3])
    c = [list(x) for x in it.comm]; c[1] = [0, NPK - 1]                          # a committee {P, -P}: its sum is infinity
    check("P and -P", c, it.msg_idx, it.sigs, [1])
    s = list(it.sigs); s[9] = bytes(len(s[9]))                                   # the all-zero signature record
    check("zero signature", it.comm, it.msg_idx, s, [9])
    c = [list(x) for x in it.comm]; c[6][100] = NPK + 1000                       # _dev only: an index past the registry
    check("index >= npk", c, it.msg_idx, it.sigs, [6], forms=("dev",), dev09=True)
    s = list(it.sigs); s[0] = it.sigs[3]; c = [list(x) for x in it.comm]; c[10] = []   # two at once, in different groups
    check("two bad items", c, it.msg_idx, s, [0, 10])


@pytest.mark.parametrize("kind", KINDS)
def test_shapes_d1_dm_m1(eng, kind):
    for sizes, d in (([2, 9, 1, 65, 3], 1), ([2, 9, 1, 65, 3], 5), ([9], 1)):
        it = Items(eng, kind, sizes, d, seed=40 + d + len(sizes))
        for form in ("host", "jac", "dev"):
            assert run_rlc(eng, it, form, it.comm, it.msg_idx, it.sigs) == ([True] * it.m, 1), (kind, sizes, d, form)
        s = list(it.sigs); s[0] = bytes(len(s[0]))
        want = [False] + [True] * (it.m - 1)
        for form in ("host", "dev"):
            assert run_rlc(eng, it, form, it.comm, it.msg_idx, s) == (want, 0), (kind, sizes, d, form)
        assert run_09(eng, it, it.comm, it.msg_idx, s) == want


@pytest.mark.parametrize("kind", KINDS)
def test_swapped_signatures_of_one_message(eng, items, kind):
    """under drawn scalars both items get verdict 0; under EQUAL caller scalars the equation holds -- the documented responsibility of a
    caller who fixes the scalars"""
    it = items[kind]
    a, b = 2, 11                                                                 # both of message 2
    assert it.msg_idx[a] == it.msg_idx[b]
    s = list(it.sigs); s[a], s[b] = it.sigs[b], it.sigs[a]
    want = [j not in (a, b) for j in range(it.m)]
    assert not it.oracle(it.comm, it.msg_idx, s, a) and not it.oracle(it.comm, it.msg_idx, s, b)
    for form in ("host", "dev"):
        assert run_rlc(eng, it, form, it.comm, it.msg_idx, s, None) == (want, 0), (kind, form)
        assert run_rlc(eng, it, form, it.comm, it.msg_idx, s, SCALARS) == (want, 0), (kind, form)    # r_a != r_b
        req = list(SCALARS); req[b] = req[a]
        assert run_rlc(eng, it, form, it.comm, it.msg_idx, s, req) == ([True] * it.m, 1), (kind, form)


def test_python_packages(eng, items):
    from bls_amd import g1pubs, g2pubs
    for mod, kind in ((g2pubs, "g2pubs"), (g1pubs, "g1pubs")):
        it = items[kind]
        keys = [mod.PublicKey(mod.Point(p, mod.PK_GROUP)) for p in it.registry]
        sigs = [mod.Signature(mod.Point(s, mod.SIG_GROUP)) for s in it.sigs]
        comms = [[keys[i] for i in c] for c in it.comm]
        msgs = [it.table[g] for g in it.msg_idx]
        assert mod.VerifyAggregateCommonBatchRandomized(sigs, comms, msgs) == [True] * it.m
        sw = list(sigs); sw[5] = sigs[8]
        want = [j != 5 for j in range(it.m)]
        assert mod.VerifyAggregateCommonBatchRandomized(sw, comms, msgs) == want == mod.VerifyAggregateCommonBatch(sw, comms, msgs)
    it = items["domain"]
    keys = [g1pubs.PublicKey(g1pubs.Point(p, 1)) for p in it.registry]
    sigs = [g1pubs.Signature(g1pubs.Point(s, 2)) for s in it.sigs]
    comms = [[keys[i] for i in c] for c in it.comm]
    msgs = [it.table[g] for g in it.msg_idx]
    assert g1pubs.VerifyAggregateCommonWithDomainBatchRandomized(sigs, comms, msgs, DOMAIN, SCALARS) == [True] * it.m
    comms[7] = []
    assert g1pubs.VerifyAggregateCommonWithDomainBatchRandomized(sigs, comms, msgs, DOMAIN) == [j != 7 for j in range(it.m)]


# ---- 3. BLSMI_LAYOUT=single: the one-lane pass 1, same verdicts ---------------------------------------------------------------------------
def test_layout_single_child(eng, items, tmp_path):
    """one fresh child process (the start-up switch is read once, at initialisation): g2pubs and g1pubs, all valid and a wrong signature"""
    W = {}
    for kind in ("g2pubs", "g1pubs"):
        it = items[kind]
        idx, off = _flat(it.comm)
        bad = list(it.sigs); bad[5] = it.sigs[8]
        W.update({kind + "_table": np.array([x.hex() for x in it.table]), kind + "_mi": np.asarray(it.msg_idx, np.uint32), kind + "_idx": idx, kind + "_off": off,
                  kind + "_reg": np.frombuffer(b"".join(it.registry), np.uint8), kind + "_sigs": np.frombuffer(b"".join(it.sigs), np.uint8),
                  kind + "_bad": np.frombuffer(b"".join(bad), np.uint8)})
    path = str(tmp_path / "workload.npz")
    np.savez(path, scalars=np.array(SCALARS, dtype=np.uint64), **W)
    env = {k: v for k, v in os.environ.items() if not k.startswith("BLSMI_") or k == "BLSMI_LIB"}
    env["BLSMI_LAYOUT"] = "single"
    out = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True, timeout=CHILD_LIMIT_S)
    assert out.returncode == 0, (out.returncode, out.stderr[-3000:])
    got = json.loads(out.stdout.strip().splitlines()[-1])
    m = len(SIZES)
    for kind in ("g2pubs", "g1pubs"):
        ok, comb, names = got[kind + "/valid"]
        assert comb == 1 and ok == [1] * m, (kind, ok, comb)
        assert "k_g2_segsum_chunk_u64" in names and "k_g2_segsum_chunk_u64_pair" not in names, (kind, names)
        assert not [x for x in names if x.startswith(PER_ITEM)], (kind, names)
        ok, comb, names = got[kind + "/bad"]
        assert comb == 0 and ok == [int(j != 5) for j in range(m)], (kind, ok, comb)
        assert "k_g2_segsum_chunk_u64" in names and "k_g2_segsum_chunk_u64_pair" not in names, (kind, names)
        assert not [x for x in names if x.endswith(("_pair", "_quad", "_row")) and x.startswith(("k_miller", "k_final_exp"))], (kind, names)


def _worker(path):
    from bls_amd import engine
    W = np.load(path)
    engine.init(0)
    scalars = [int(x) for x in W["scalars"]]
    out = {}
    for kind in ("g2pubs", "g1pubs"):
        table = [bytes.fromhex(str(x)) for x in W[kind + "_table"]]
        fn = getattr(engine, kind + "_verify_aggregate_common_batch_rlc")
        for case, sigs in (("valid", W[kind + "_sigs"]), ("bad", W[kind + "_bad"])):
            (ok, _, comb), names = names_of(engine, lambda: fn(table, W[kind + "_mi"], W[kind + "_reg"].tobytes(), NPK, W[kind + "_idx"], W[kind + "_off"], sigs.tobytes(), scalars))
            out["%s/%s" % (kind, case)] = ([int(x) for x in ok], comb, names)
    print(json.dumps(out))


if __name__ == "__main__":
    _worker(sys.argv[1])
