"""-m gpu: committee batches (blsmi 0.9).  Segmented sums bit for bit against the oracle's sums of the gathered points, and batches of
VerifyAggregateCommon whose every verdict equals the oracle's (and, for a sample, the single-call entry point's).  Valid aggregates are made
cheaply by signing with the committee's summed secret key: sig = (sum sk mod r) H(m) (tests/test_agg_common_batch_cpu.py)."""
import hashlib
import threading

import numpy as np
import pytest

from gpu_common import P, RC, g1_to_jac, g2_to_jac, jac1, jac2

pytestmark = pytest.mark.gpu

PB = {1: 96, 2: 192}
DOM = b"\x07\x00\x00\x00\x01\x00\x00\x00"


@pytest.fixture(scope="module")
def eng():
    from bls_amd import engine
    engine.init(0)
    yield engine
    engine.set_option("segsum_chunk", 0)


def _dev():
    import torch
    return torch.device("cuda", 0)


def _t(b, dtype=np.uint8):
    import torch
    a = np.frombuffer(bytes(b), dtype=np.uint8).copy() if not isinstance(b, np.ndarray) else np.ascontiguousarray(b)
    if a.size == 0:
        a = np.zeros(8, dtype=np.uint8)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(_dev())


def _sks(seed, n):
    """n secret scalars below r (big-endian 32 bytes each) as an (n, 32) uint8 array"""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 0] &= 0x3f
    return s


def _neg(p, group):
    if p is None:
        return None
    if group == 1:
        return p[:48] + ((P.Q - int.from_bytes(p[48:], "big")) % P.Q).to_bytes(48, "big")
    return p[:96] + b"".join(((P.Q - int.from_bytes(p[o:o + 48], "big")) % P.Q).to_bytes(48, "big") for o in (96, 144))


def _registry(eng, group, n, seed):
    sk = _sks(seed, n)
    pts, _ = (eng.g1_mul_generator_batch if group == 1 else eng.g2_mul_generator_batch)(sk.reshape(-1).tobytes(), n)
    return sk, [bytes(pts[i]) for i in range(n)]


def _oracle_sum(group, table, seg, inf=None):
    n = len(seg)
    if n == 0:
        return None
    flags = bytes(inf[i] for i in seg) if inf is not None else None
    return (RC.g1_sum if group == 1 else RC.g2_sum)(b"".join(table[i] for i in seg), n, flags)


# ---- 1. segmented sums ----------------------------------------------------------------------------------------------------------
def _sum_case(eng, group):
    xs = P.XORShift(100 + group)
    rng = np.random.default_rng(group)
    _, keys = _registry(eng, group, 700, 7 + group)
    table = keys + [_neg(keys[0], group)]                                    # the last key is -keys[0]
    npk = len(table)
    inf = np.zeros(npk, dtype=np.uint8)
    inf[[5, 6, 7]] = 1                                                       # keys flagged infinite (affine form: in_inf)
    segs = [list(rng.integers(0, npk, size=L)) for L in (0, 1, 2, 63, 64, 65, 513, 5000)]
    segs += [[3] * 100, [0, npk - 1], [5, 6], [9, 9, 10, 5, 9], [], [0, npk - 1, 11]]
    idx = np.array([i for s in segs for i in s], dtype=np.uint32)
    off = eng.seg_offsets([len(s) for s in segs])
    want = [_oracle_sum(group, table, s, inf) for s in segs]
    jtab = [(jac1 if group == 1 else jac2)(xs, table[i]) if not inf[i] else (g1_to_jac if group == 1 else g2_to_jac)(None) for i in range(npk)]
    return table, jtab, inf, segs, idx, off, want


@pytest.mark.parametrize("group", [1, 2])
def test_segmented_sums_match_the_oracle(eng, group):
    pb = PB[group]
    table, jtab, inf, segs, idx, off, want = _sum_case(eng, group)
    npk = len(table)
    aff, jac = (eng.g1_sum_segmented, eng.g1_sum_segmented_jac) if group == 1 else (eng.g2_sum_segmented, eng.g2_sum_segmented_jac)
    results = []
    try:
        for K in (1, 0, 1024):
            eng.set_option("segsum_chunk", K)
            out, oinf = aff(b"".join(table), npk, idx, off, inf)
            for j, w in enumerate(want):
                assert oinf[j] == (1 if w is None else 0), (K, j)
                assert out[pb * j:pb * (j + 1)] == (bytes(pb) if w is None else w), (K, j)
            jo, ji = jac(b"".join(jtab), npk, idx, off)
            assert jo == out and np.array_equal(ji, oinf), K
            results.append(out)
    finally:
        eng.set_option("segsum_chunk", 0)
    assert results[0] == results[1] == results[2]
    # idx = NULL: consecutive runs of the table
    sizes = [0, 1, 65, 130, 0, 3]
    o2, i2 = aff(b"".join(table[:sum(sizes)]), sum(sizes), None, eng.seg_offsets(sizes), inf[:sum(sizes)])
    at = 0
    for j, L in enumerate(sizes):
        w = _oracle_sum(group, table, list(range(at, at + L)), inf)
        assert o2[pb * j:pb * (j + 1)] == (bytes(pb) if w is None else w) and i2[j] == (w is None), j
        at += L


@pytest.mark.parametrize("group", [1, 2])
def test_segmented_sums_dev(eng, group):
    import torch
    pb = PB[group]
    table, _, inf, segs, idx, off, want = _sum_case(eng, group)
    npk, m = len(table), len(segs)
    grp = "g1" if group == 1 else "g2"
    d_p, d_f, d_x, d_o = _t(b"".join(table)), _t(inf), _t(idx), _t(off)
    d_out = torch.zeros(pb * m, dtype=torch.uint8, device=_dev()); d_inf = torch.zeros(m, dtype=torch.uint8, device=_dev())
    eng.sum_segmented_dev(grp, d_p.data_ptr(), d_f.data_ptr(), npk, d_x.data_ptr(), d_o.data_ptr(), m, d_out.data_ptr(), d_inf.data_ptr())
    out, oinf = d_out.cpu().numpy().tobytes(), d_inf.cpu().numpy()
    for j, w in enumerate(want):
        assert oinf[j] == (w is None) and out[pb * j:pb * (j + 1)] == (bytes(pb) if w is None else w), j
    # an index past the table marks only its own segment: out_inf = 2, record zeroed, nothing read beyond npk
    bad = idx.copy()
    k = int(off[3]) + 5                                                      # inside segment 3 (63 keys)
    bad[k] = npk + 1000
    d_x2 = _t(bad)
    eng.sum_segmented_dev(grp, d_p.data_ptr(), d_f.data_ptr(), npk, d_x2.data_ptr(), d_o.data_ptr(), m, d_out.data_ptr(), d_inf.data_ptr())
    out2, oinf2 = d_out.cpu().numpy().tobytes(), d_inf.cpu().numpy()
    assert oinf2[3] == 2 and out2[pb * 3:pb * 4] == bytes(pb)
    for j in range(m):
        if j != 3:
            assert oinf2[j] == oinf[j] and out2[pb * j:pb * (j + 1)] == out[pb * j:pb * (j + 1)], j


# ---- 2. verdicts --------------------------------------------------------------------------------------------------------------
KINDS = ["g2pubs", "g1pubs", "g1pubs_domain"]


class Batch:
    """m items over one registry, rotated corruptions; .want: the oracle's verdicts"""

    def __init__(self, eng, kind, sizes, seed, npk=None):
        self.kind = kind
        self.pkg = RC.g2pubs if kind == "g2pubs" else RC.g1pubs
        self.kg, self.sg = (2, 1) if kind == "g2pubs" else (1, 2)
        rng = np.random.default_rng(seed)
        m = len(sizes)
        npk = npk or max(64, max(sizes) + 8)
        self.sk, keys = _registry(eng, self.kg, npk, seed)
        self.table = keys + [_neg(keys[0], self.kg)]
        self.npk = len(self.table)
        ski = [int.from_bytes(self.sk[i].tobytes(), "big") for i in range(npk)] + [(-int.from_bytes(self.sk[0].tobytes(), "big")) % P.R_ORDER]
        comm = [list(rng.integers(0, npk, size=L)) for L in sizes]
        if kind == "g1pubs_domain":
            msgs = [hashlib.sha256(b"item %d %d" % (seed, j)).digest() for j in range(m)]
        else:
            msgs = [b"attestation %d/%d" % (seed, j) + b"x" * (j % 7) for j in range(m)]
        sign_msgs = list(msgs)
        for j in range(m):                                                   # rotated corruptions
            c = j % 9
            if c == 1:
                sign_msgs[j] = msgs[j][:-1] + bytes([msgs[j][-1] ^ 1])       # signed another message
            elif c == 2 and len(comm[j]) > 1:
                comm[j] = comm[j] + [int(rng.integers(0, npk))]              # one extra member (signature over the others)
            elif c == 7 and comm[j]:
                comm[j] = comm[j] + [comm[j][0]]                             # repeated index, signed with it: valid
            elif c == 8:
                comm[j] = [0, npk] + (comm[j][:1] if j % 18 == 17 else [])  # P and -P: the sum is infinity (with a third key: valid)
        signers = [list(c) for c in comm]
        for j in range(m):
            if j % 9 == 2 and len(comm[j]) > 1:
                signers[j] = comm[j][:-1]
            if j % 9 == 3 and len(comm[j]) > 1:
                comm[j] = comm[j][:-1]                                       # one member dropped after signing
        ssum = [(sum(ski[i] for i in s) % P.R_ORDER).to_bytes(32, "big") for s in signers]
        ssum = [s if int.from_bytes(s, "big") else (1).to_bytes(32, "big") for s in ssum]
        if kind == "g2pubs":
            sigs, _ = eng.g2pubs_sign_batch(sign_msgs, b"".join(ssum))
        elif kind == "g1pubs":
            sigs, _ = eng.g1pubs_sign_batch(sign_msgs, b"".join(ssum))
        else:
            sigs, _ = eng.g1pubs_sign_with_domain_batch(sign_msgs, DOM, b"".join(ssum))
        sigs = [bytes(s) for s in sigs]
        for j in range(m):
            c = j % 9
            if c == 4 and m > 1:
                sigs[j] = sigs[(j + 1) % m]                                  # another committee's signature
            elif c == 5:
                sigs[j] = _neg(sigs[j], self.sg)
            elif c == 6:
                sigs[j] = bytes(PB[self.sg])                                 # the all-zero record
        if m > 2:
            comm[-1] = []                                                    # an empty committee
        self.comm, self.msgs, self.sigs, self.m = comm, msgs, sigs, m
        self.idx = np.array([i for c in comm for i in c], dtype=np.uint32)
        self.off = np.zeros(m + 1, dtype=np.uint64)
        self.off[1:] = np.cumsum([len(c) for c in comm])

    def oracle(self, j):
        pks = [self.table[i] for i in self.comm[j]]
        sig = self.sigs[j]
        if not any(sig):
            return False
        if self.kind == "g1pubs_domain":
            return bool(pks) and self.pkg.verify_aggregate_common_with_domain(sig, pks, self.msgs[j], DOM)
        return self.pkg.verify_aggregate_common(sig, pks, self.msgs[j])

    def want(self):
        return [self.oracle(j) for j in range(self.m)]

    def run(self, eng, form="affine"):
        k = self.kind
        if form == "dev":
            import torch
            d_pk, d_x, d_off, d_s = _t(b"".join(self.table)), _t(self.idx), _t(self.off), _t(b"".join(self.sigs))
            if k == "g1pubs_domain":
                d_m, d_mo = _t(b"".join(self.msgs)), _t(DOM)
            else:
                mo = np.zeros(self.m + 1, dtype=np.uint64); mo[1:] = np.cumsum([len(x) for x in self.msgs])
                d_m, d_mo = _t(b"".join(self.msgs)), _t(mo)
            d_ok = torch.zeros(self.m, dtype=torch.uint8, device=_dev())
            eng.verify_aggregate_common_batch_dev("g2pubs" if k == "g2pubs" else "g1pubs", d_m.data_ptr(), d_mo.data_ptr(), d_pk.data_ptr(), self.npk,
                                                  d_x.data_ptr(), d_off.data_ptr(), d_s.data_ptr(), d_ok.data_ptr(), self.m, domain=(k == "g1pubs_domain"))
            return [bool(x) for x in d_ok.cpu().numpy()]
        if form == "jac":
            xs = P.XORShift(5)
            keys = b"".join((jac1 if self.kg == 1 else jac2)(xs, p) for p in self.table)
            sigs = b"".join((jac1 if self.sg == 1 else jac2)(xs, s) if any(s) else (g1_to_jac if self.sg == 1 else g2_to_jac)(None) for s in self.sigs)
            if k == "g2pubs":
                ok, bm = eng.g2pubs_verify_aggregate_common_batch_jac(self.msgs, keys, self.npk, self.idx, self.off, sigs)
            elif k == "g1pubs":
                ok, bm = eng.g1pubs_verify_aggregate_common_batch_jac(self.msgs, keys, self.npk, self.idx, self.off, sigs)
            else:
                ok, bm = eng.g1pubs_verify_aggregate_common_with_domain_batch_jac(b"".join(self.msgs), DOM, keys, self.npk, self.idx, self.off, sigs)
        else:
            keys, sigs = b"".join(self.table), b"".join(self.sigs)
            if k == "g2pubs":
                ok, bm = eng.g2pubs_verify_aggregate_common_batch(self.msgs, keys, self.npk, self.idx, self.off, sigs)
            elif k == "g1pubs":
                ok, bm = eng.g1pubs_verify_aggregate_common_batch(self.msgs, keys, self.npk, self.idx, self.off, sigs)
            else:
                ok, bm = eng.g1pubs_verify_aggregate_common_with_domain_batch(b"".join(self.msgs), DOM, keys, self.npk, self.idx, self.off, sigs)
        assert np.array_equal(np.packbits(ok.astype(bool), bitorder="little")[:len(bm)], bm)
        return [bool(x) for x in ok]

    def single(self, eng, j):
        pks = b"".join(self.table[i] for i in self.comm[j])
        n = len(self.comm[j])
        if self.kind == "g2pubs":
            return eng.g2pubs_verify_aggregate_common(self.msgs[j], pks, self.sigs[j], n)
        if self.kind == "g1pubs":
            return eng.g1pubs_verify_aggregate_common(self.msgs[j], pks, self.sigs[j], n)
        return eng.g1pubs_verify_aggregate_common_with_domain(self.msgs[j], DOM, pks, self.sigs[j], n)


@pytest.mark.parametrize("kind", KINDS)
def test_verdicts_equal_the_oracle(eng, kind):
    rng = np.random.default_rng(11)
    shapes = [[5], [9, 1, 2, 3, 64, 65, 0], [128] * 128, list(rng.integers(0, 601, size=20)) + [0, 600]]
    for si, sizes in enumerate(shapes):
        b = Batch(eng, kind, sizes, seed=31 * si + KINDS.index(kind))
        want = b.want()
        if b.m > 1:
            assert any(want) and not all(want), (kind, si)
        for form in ("affine", "jac", "dev"):
            assert b.run(eng, form) == want, (kind, si, form)
        for j in range(min(b.m, 9)):
            assert b.single(eng, j) == want[j], (kind, si, j)


# ---- 3. routing: the m checks run in the layout m picks ------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1000, 2048, 4096])
def test_routing_sizes(eng, m):
    rng = np.random.default_rng(m)
    b = Batch(eng, "g2pubs", list(rng.integers(1, 4, size=m)), seed=m, npk=256)
    got = b.run(eng)
    sample = list(range(0, m, max(1, m // 40))) + [m - 1]
    for j in sample:
        assert got[j] == b.oracle(j), j
    assert all(got[j] for j in range(m - 1) if j % 9 in (0, 7))             # by construction: valid ...
    assert not any(got[j] for j in range(m) if j % 9 in (1, 4, 5, 6) or j % 18 == 8) and not got[m - 1]   # ... and not


# ---- 4. size: a 2^20-key registry resident on the device ---------------------------------------------------------------------
def test_registry_of_a_million_keys(eng):
    import torch
    n = 1 << 20
    sk = _sks(2024, n)
    keys, _ = eng.g1_mul_generator_batch(sk.reshape(-1).tobytes(), n)
    rng = np.random.default_rng(3)
    comm = [rng.integers(0, n, size=512).astype(np.uint32) for _ in range(128)] + [rng.integers(0, n, size=1 << 17).astype(np.uint32)]
    m = len(comm)
    ski = np.array([int.from_bytes(sk[i].tobytes(), "big") for i in range(n)], dtype=object)
    ssum = [(int(ski[c].sum()) % P.R_ORDER).to_bytes(32, "big") for c in comm]
    msgs = [hashlib.sha256(b"slot %d" % j).digest() for j in range(m)]
    sigs, _ = eng.g1pubs_sign_with_domain_batch(msgs, DOM, b"".join(ssum))
    sigs = sigs.copy()
    sigs[17] = sigs[18]                                                      # one corrupted item
    idx = np.concatenate(comm)
    off = eng.seg_offsets([len(c) for c in comm])
    d_pk, d_x, d_off, d_s, d_m, d_d = _t(keys.reshape(-1)), _t(idx), _t(off), _t(sigs.reshape(-1)), _t(b"".join(msgs)), _t(DOM)
    d_ok = torch.zeros(m, dtype=torch.uint8, device=_dev())
    eng.verify_aggregate_common_batch_dev("g1pubs", d_m.data_ptr(), d_d.data_ptr(), d_pk.data_ptr(), n, d_x.data_ptr(), d_off.data_ptr(),
                                          d_s.data_ptr(), d_ok.data_ptr(), m, domain=True)
    ok = d_ok.cpu().numpy()
    assert ok[17] == 0 and all(ok[j] == 1 for j in range(m) if j != 17)
    d_out = torch.zeros(96 * m, dtype=torch.uint8, device=_dev()); d_inf = torch.zeros(m, dtype=torch.uint8, device=_dev())
    eng.sum_segmented_dev("g1", d_pk.data_ptr(), None, n, d_x.data_ptr(), d_off.data_ptr(), m, d_out.data_ptr(), d_inf.data_ptr())
    out = d_out.cpu().numpy().tobytes()
    for j in (0, 77, m - 1):
        assert out[96 * j:96 * (j + 1)] == RC.g1_sum(keys[comm[j]].reshape(-1).tobytes(), len(comm[j])), j


# ---- 5. concurrency ------------------------------------------------------------------------------------------------------------
def test_concurrent_batches(eng):
    batches = [Batch(eng, KINDS[i % 3], [32 + 9 * i] * 16, seed=500 + i) for i in range(4)]
    alone = [b.run(eng) for b in batches]
    got = [None] * 4

    def work(i):
        for _ in range(3):
            r = batches[i].run(eng)
            if got[i] is None or r != alone[i]:
                got[i] = r

    th = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert got == alone
    assert alone[0] == batches[0].want()
