"""-m gpu: the compressed wire format <-> the reference's in-memory points (blsmi 0.15: blsmi_g?_decompress_batch_jac[_dev],
blsmi_g?_compress_batch_jac[_dev]), record for record against oracle.pyref on the corpora of tests/wire_jac_cases.py, both groups, host and
device-pointer forms: every decompression route (the kernel that writes the in-memory record itself; the small-call routes that finish with
k_affine_to_jac) gives the same bytes as blsmi_g?_decompress_batch + ToProjective; the one-launch compression gives the bytes of
jac_to_affine_batch + compress_batch with every z pattern laid out against the wave; the round trip; decompression chained on the device
into the *_jac_dev consumers; and VerifySerializedBatchRandomized of both packages.  (tests/test_gpu_wire_jac_single.py runs this file's G2
compression checks in a child process under BLSMI_LAYOUT=single.)

The tests send bad POINTS, never bad buffers: every record is full size and in bounds."""
import ctypes

import numpy as np
import pytest

import point_check_cases as K
import wire_jac_cases as W
from gpu_common import P, RC, jac1, jac2, sk_bytes

pytestmark = pytest.mark.gpu

GROUPS = (1, 2)
NAME = {1: "g1", 2: "g2"}
CHECKS = (1, 2, 0)
POISON = 0xA5
PAD = 64
LAT_DEFAULT = 8192
WAVE_MAX = 512                                                               # route.h: swu_wave_max, the check-0 calls one wave per point serves
DECOMPRESS_SIZES = (1, 63, 64, 65, 130)
COMPRESS_SIZES = {1: (1, 63, 64, 65), 2: (1, 33, 64, 65)}                   # (33: one more than the 32 points of a lane-pair workgroup, the form that was measured and dropped)


@pytest.fixture(scope="module")
def eng():
    from bls_amd import engine
    engine.init(0)
    return engine


class Profile:
    """the kernel names of the calls made inside the block, in launch order"""

    def __init__(self, eng):
        self.lib = eng._lib()
        self.names = []

    def __enter__(self):
        buf = ctypes.create_string_buffer(1 << 14)
        self.lib.blsmi_last_profile(buf, ctypes.c_size_t(len(buf)))           # (read-and-clear)
        self.lib.blsmi_set_profiling(1)
        return self

    def __exit__(self, *exc):
        buf = ctypes.create_string_buffer(1 << 14)
        self.lib.blsmi_last_profile(buf, ctypes.c_size_t(len(buf)))
        self.lib.blsmi_set_profiling(0)
        names = [item.rsplit("=", 1)[0].strip() for item in buf.value.decode().split(";") if item]
        self.names = [k for k in names if not k.startswith("(")]               # ("(between)": the time after a call's last kernel, no kernel)
        return False


def _dev(b):
    import torch
    a = np.ascontiguousarray(b) if isinstance(b, np.ndarray) else np.frombuffer(bytes(b), dtype=np.uint8)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(torch.device("cuda", 0))


def _poisoned(nbytes):
    import torch
    return torch.full((nbytes + 2 * PAD,), POISON, dtype=torch.uint8, device=torch.device("cuda", 0))


def _inside(d, nbytes):
    """the payload of a poisoned buffer, after checking the bytes around it"""
    a = d.cpu().numpy()
    assert (a[:PAD] == POISON).all() and (a[PAD + nbytes:] == POISON).all(), "bytes outside the buffer were written"
    return a[PAD:PAD + nbytes].copy()


# ---- decompression -----------------------------------------------------------------------------------------------------------------------
def _decompress_affine(eng, group, blob, n, check):
    return (eng.g1_decompress_batch if group == 1 else eng.g2_decompress_batch)(blob, n, check)


def _decompress_host(eng, group, blob, n, check):
    return (eng.g1_decompress_batch_jac if group == 1 else eng.g2_decompress_batch_jac)(blob, n, check)


def _decompress_resident(eng, group, blob, n, check, want_inf=True):
    import torch
    jb = 8 * W.JW[group]
    d_in = _dev(blob)
    d_out, d_inf, d_err = _poisoned(jb * n), _poisoned(n), _poisoned(n)
    eng.decompress_batch_jac_dev(NAME[group], d_in.data_ptr(), n, d_out.data_ptr() + PAD, d_inf.data_ptr() + PAD if want_inf else 0, d_err.data_ptr() + PAD, check)
    torch.cuda.synchronize()
    assert d_in.cpu().numpy().tobytes() == bytes(blob), "the _dev form wrote to its input"
    inf = _inside(d_inf, n)
    assert want_inf or (inf == POISON).all()
    return _inside(d_out, jb * n).reshape(n, jb), inf.astype(bool), _inside(d_err, n)


def _check_decompression(eng, group, cs, check, got, where):
    """got = (records, inf, err) of a decompress_batch_jac form against the affine call on the same bytes AND against the oracle"""
    n = len(cs)
    blob = b"".join(c.blob for c in cs)
    rec, inf, err = got
    arec, ainf, aerr = _decompress_affine(eng, group, blob, n, check)
    assert err.tolist() == aerr.tolist() and inf.tolist() == ainf.tolist(), (where, check)
    for i, c in enumerate(cs):
        want_err, want_inf, a = W.expect(group, c, check)
        assert (int(err[i]), int(inf[i])) == (want_err, want_inf), (where, check, i, c.label)
        model = W.wire_record_as_memory(group, arec[i], aerr[i] or ainf[i])   # the in-memory form of the affine call's record
        assert rec[i].tobytes() == model.tobytes(), (where, check, i, c.label, "differs from the affine call's record")
        assert rec[i].tobytes() == W.memory_record(group, a).tobytes(), (where, check, i, c.label, "differs from the oracle")


@pytest.mark.parametrize("group", GROUPS)
def test_decompression_corpus_every_check_host_and_resident(eng, group):
    cs = W.encodings(group)
    n = len(cs)
    blob = b"".join(c.blob for c in cs)
    for check in CHECKS:
        _check_decompression(eng, group, cs, check, _decompress_host(eng, group, blob, n, check), "host")
        _check_decompression(eng, group, cs, check, _decompress_resident(eng, group, blob, n, check), "resident")
    rec, _, err = _decompress_resident(eng, group, blob, n, 1, want_inf=False)  # the flags are optional
    host = _decompress_host(eng, group, blob, n, 1)
    assert rec.tobytes() == host[0].tobytes() and err.tolist() == host[2].tolist()


def _fused_only(names, group):
    return names == ["k_%s_decompress_jac" % NAME[group]]


@pytest.mark.parametrize("n", DECOMPRESS_SIZES + (WAVE_MAX + 1,))
@pytest.mark.parametrize("group", GROUPS)
def test_decompression_sizes_and_routes_give_the_same_bytes(eng, group, n):
    """default thresholds: the small-call routes (check 0: a wave per point; check 1: the level program) + k_affine_to_jac; latency threshold
    0: the kernel that writes the in-memory record itself (check 0: from WAVE_MAX + 1 points on).  Same bytes."""
    cs = W.take(W.encodings(group), n, start=3 * n)
    blob = b"".join(c.blob for c in cs)
    checks = CHECKS if n <= max(DECOMPRESS_SIZES) else (0,)
    small = {}
    for check in checks:
        with Profile(eng) as prof:
            small[check] = _decompress_host(eng, group, blob, n, check)
        _check_decompression(eng, group, cs, check, small[check], "default thresholds")
        if check == 2 or n > WAVE_MAX:
            assert _fused_only(prof.names, group), prof.names
        else:
            assert "k_affine_to_jac" in prof.names and "k_%s_decompress_jac" % NAME[group] not in prof.names, prof.names
    eng.set_latency_threshold(0)
    try:
        for check in checks:
            with Profile(eng) as prof:
                got = _decompress_host(eng, group, blob, n, check)
            if check or n > WAVE_MAX:
                assert _fused_only(prof.names, group), (check, prof.names)
            for a, b in zip(got, small[check]):
                assert a.tobytes() == b.tobytes(), (check, "the routes differ")
            res = _decompress_resident(eng, group, blob, n, check)
            for a, b in zip(res, small[check]):
                assert a.tobytes() == b.tobytes(), (check, "the resident form differs")
    finally:
        eng.set_latency_threshold(LAT_DEFAULT)


@pytest.mark.parametrize("group", GROUPS)
def test_decompression_against_pyref_directly(eng, group):
    """the well-formed records: oracle.pyref.g?_decompress + to_mont, no library call on the expectation's side"""
    cs = [c for c in W.encodings(group) if c.err == 0 and not c.outside]
    rec, inf, err = _decompress_host(eng, group, b"".join(c.blob for c in cs), len(cs), 1)
    assert not err.any()
    for i, c in enumerate(cs):
        a = (P.g1_decompress if group == 1 else P.g2_decompress)(c.blob)
        assert bool(inf[i]) == (a is None)
        coords = [0, 1, 0] if a is None else [a[0], a[1], 1]
        if group == 2:
            coords = [v for c2 in ([(0, 0), (1, 0), (0, 0)] if a is None else [a[0], a[1], (1, 0)]) for v in c2]
        want = np.array([w for v in coords for w in P.limbs64(P.to_mont(v))], dtype=np.uint64)
        assert rec[i].tobytes() == want.tobytes(), (i, c.label)


# ---- compression -------------------------------------------------------------------------------------------------------------------------
def _compress_host(eng, group, recs):
    return (eng.g1_compress_batch_jac if group == 1 else eng.g2_compress_batch_jac)(recs.tobytes(), recs.shape[0])


def _compress_two_calls(eng, group, recs):
    n = recs.shape[0]
    aff, inf = (eng.g1_jac_to_affine_batch if group == 1 else eng.g2_jac_to_affine_batch)(recs.tobytes(), n)
    return (eng.g1_compress_batch if group == 1 else eng.g2_compress_batch)(aff, n, inf.astype(np.uint8))


def _compress_resident(eng, group, recs):
    import torch
    n = recs.shape[0]
    d_in = _dev(recs.tobytes())
    d_out = _poisoned(W.WB[group] * n)
    eng.compress_batch_jac_dev(NAME[group], d_in.data_ptr(), n, d_out.data_ptr() + PAD)
    torch.cuda.synchronize()
    assert d_in.cpu().numpy().tobytes() == recs.tobytes(), "the _dev form wrote to its input"
    return _inside(d_out, W.WB[group] * n).reshape(n, W.WB[group])


def compression_results(eng, group, resident=True):
    """{case: the compressed bytes (hex) of the one-call form} for the whole corpus and the ragged sizes, every output checked against the
    oracle, the two-call route and (resident) the device-pointer form; and the kernel names the calls' profiles carried"""
    out, names = {}, set()
    cases = [("corpus",) + W.compression_corpus(group)] + [("n%d" % n,) + W.compression_cut(group, n) for n in COMPRESS_SIZES[group]]
    for label, recs, want in cases:
        with Profile(eng) as prof:
            got = _compress_host(eng, group, recs)
        assert len(prof.names) == 1, (label, prof.names)                      # one launch for every n
        names |= set(prof.names)
        assert got.shape == (recs.shape[0], W.WB[group])
        bad = [i for i in range(recs.shape[0]) if got[i].tobytes() != want[i]]
        assert not bad, (NAME[group], label, bad[:8], got[bad[0]].tobytes().hex(), want[bad[0]].hex())
        assert got.tobytes() == _compress_two_calls(eng, group, recs).tobytes(), (NAME[group], label, "differs from the two-call route")
        assert not resident or got.tobytes() == _compress_resident(eng, group, recs).tobytes(), (NAME[group], label, "the resident form differs")
        out[label] = got.tobytes().hex()
    return out, sorted(names)


@pytest.mark.parametrize("group", GROUPS)
def test_compression_corpus_and_ragged_sizes(eng, group):
    _, names = compression_results(eng, group)
    assert names == ["k_%s_compress_jac" % NAME[group]], names


@pytest.mark.parametrize("group", GROUPS)
def test_round_trip(eng, group):
    """compress_batch_jac(decompress_batch_jac(b)) == b for every well-formed b (an x field that is not below q is not: it is read as 0)"""
    formed = [c for c in W.encodings(group) if c.err == 0 and c.label != "x >= q"]
    for check, cs in ((1, [c for c in formed if not c.outside]), (0, formed)):   # (check 0: the curve points outside the subgroup come back too)
        assert any(c.inf for c in cs) and any(c.blob[0] & 0x20 for c in cs) and (check or any(c.outside for c in cs))
        blob = b"".join(c.blob for c in cs)
        rec, _, err = _decompress_host(eng, group, blob, len(cs), check)
        assert not err.any()
        assert _compress_host(eng, group, rec.view(np.uint64)).tobytes() == blob, check


# ---- chaining on the device --------------------------------------------------------------------------------------------------------------
N_CHAIN = 66


def _signed(pkg, n, xs):
    """n (message, compressed key, compressed signature) tuples of one package, from six distinct signers"""
    R = RC.g2pubs if pkg == "g2pubs" else RC.g1pubs
    pk_group, sig_group = (2, 1) if pkg == "g2pubs" else (1, 2)
    base = []
    for i in range(6):
        sk = sk_bytes(xs)
        m = b"wire tuple %d" % i
        base.append((m, W.compress(pk_group, W.G.unwire(pk_group, R.priv_to_pub(sk))), W.compress(sig_group, W.G.unwire(sig_group, R.sign(m, sk)))))
    t = [base[i % 6] for i in range(n)]
    return [x[0] for x in t], [x[1] for x in t], [x[2] for x in t]


def _first(group, **kw):
    return next(c for c in W.encodings(group) if all(getattr(c, k) == v for k, v in kw.items()))


def test_decompression_chained_into_verify_and_check_on_the_device(eng):
    import torch
    dev = torch.device("cuda", 0)
    n = N_CHAIN
    msgs, pkb, sgb = _signed("g2pubs", n, P.XORShift(9560))
    want = [True] * n
    sgb[7] = W.compress(1, W.G.neg(1, P.g1_decompress(sgb[7]))); want[7] = False          # a negated signature: decodes, does not verify
    pkb[20] = _first(2, err=3).blob; want[20] = False                                     # an x with no y
    sgb[41] = _first(1, outside=True).blob; want[41] = False                              # a curve point outside the subgroup
    pkb[65] = _first(2, inf=1).blob; want[65] = False                                     # a well-formed infinity
    pm = eng.PackedMsgs(msgs)
    d_m = torch.from_numpy(pm.buf.copy()).to(dev); d_o = torch.from_numpy(pm.off.view(np.int64).copy()).to(dev)
    d_pk, d_sg = _poisoned(288 * n), _poisoned(144 * n)
    d_epk, d_esg = _poisoned(n), _poisoned(n)
    d_pkb, d_sgb = _dev(b"".join(pkb)), _dev(b"".join(sgb))
    eng.decompress_batch_jac_dev("g2", d_pkb.data_ptr(), n, d_pk.data_ptr() + PAD, 0, d_epk.data_ptr() + PAD, 1)
    eng.decompress_batch_jac_dev("g1", d_sgb.data_ptr(), n, d_sg.data_ptr() + PAD, 0, d_esg.data_ptr() + PAD, 1)
    assert [i for i, e in enumerate(_inside(d_epk, n)) if e] == [20] and [i for i, e in enumerate(_inside(d_esg, n)) if e] == [41]
    d_ok = torch.full((n,), POISON, dtype=torch.uint8, device=dev)
    eng.verify_batch_jac_dev("g2pubs", d_m.data_ptr(), d_o.data_ptr(), d_pk.data_ptr() + PAD, d_sg.data_ptr() + PAD, d_ok.data_ptr(), n)
    assert d_ok.cpu().numpy().tolist() == [1 if w else 0 for w in want]
    assert want[0] == RC.g2pubs.verify(msgs[0], W.G.wire(2, P.g2_decompress(pkb[0])), W.G.wire(1, P.g1_decompress(sgb[0])))
    for name, d_pts, bad in (("g2", d_pk, (20, 65)), ("g1", d_sg, (41,))):
        d_st = _poisoned(n)
        eng.check_batch_dev(name, d_pts.data_ptr() + PAD, 0, n, d_st.data_ptr() + PAD, jac=True, check=1)
        torch.cuda.synchronize()
        assert _inside(d_st, n).tolist() == [K.INFINITY if i in bad else K.OK for i in range(n)]   # an undecodable element IS the zero point
    _inside(d_pk, 288 * n); _inside(d_sg, 144 * n)


# ---- VerifySerializedBatchRandomized -----------------------------------------------------------------------------------------------------
def _blocks_with(n, block, bad):
    return sum(min(n, lo + block) - lo for lo in range(0, n, block) if any(lo <= i < lo + block for i in bad))


@pytest.mark.parametrize("pkg", ("g2pubs", "g1pubs"))
def test_verify_serialized_batch_randomized(eng, pkg):
    import importlib
    from bls_amd import _groups
    mod = importlib.import_module("bls_amd." + pkg)
    pk_group, sig_group = (2, 1) if pkg == "g2pubs" else (1, 2)
    n, block = N_CHAIN, 2
    msgs, pkb, sgb = _signed(pkg, n, P.XORShift(9570 + pk_group))
    dec = {1: P.g1_decompress, 2: P.g2_decompress}
    runs = [(list(pkb), list(sgb), set())]
    s = list(sgb); s[13] = W.compress(sig_group, W.G.neg(sig_group, dec[sig_group](s[13])))
    runs.append((list(pkb), s, {13}))
    p, s = list(pkb), list(sgb)
    p[30] = _first(pk_group, err=3).blob; s[51] = _first(sig_group, outside=True).blob
    runs.append((p, s, {30, 51}))
    for p, s, bad in runs:
        want = [i not in bad for i in range(n)]
        assert mod.VerifySerializedBatchRandomized(msgs, p, s, block=block) == want, (pkg, sorted(bad))
        assert mod.VerifySerializedBatch(msgs, p, s) == want, (pkg, sorted(bad))
        ok, _, combined, rechecked = _groups.verify_serialized_randomized(pkg, pk_group, sig_group, msgs, p, s, block)
        assert [bool(x) for x in ok] == want and combined == (0 if bad else 1)
        assert rechecked == _blocks_with(n, block, bad), (pkg, sorted(bad), rechecked)


def test_batch_deserialize_and_serialize_mirrors(eng):
    from bls_amd import g1pubs, g2pubs
    for mod, pk_group, sig_group in ((g2pubs, 2, 1), (g1pubs, 1, 2)):
        for group, des, ser in ((pk_group, mod.DeserializePublicKeys, mod.SerializePublicKeys), (sig_group, mod.DeserializeSignatures, mod.SerializeSignatures)):
            cs = W.encodings(group)
            objs, errs = des([c.blob for c in cs])
            assert errs == [W.expect(group, c, 1)[0] for c in cs]
            assert [o is None for o in objs] == [e != 0 for e in errs]
            good = [(o, c) for o, c in zip(objs, cs) if o is not None]
            assert ser([o for o, _ in good]) == [c.blob for _, c in good]
            assert good[0][0].Serialize() == good[0][1].blob                   # one object: the same bytes, one call
    xs = P.XORShift(9580)
    w = [W.G.wire(1, a) for a in W.G.subgroup_points(1)[:3]]
    mixed = [g2pubs.NewSignatureFromG1Projective(jac1(xs, w[0])), g2pubs.NewSignatureFromG1(w[1]), g2pubs.NewAggregateSignature(), g2pubs.NewSignatureFromG1Projective(jac1(xs, w[2]))]
    assert g2pubs.SerializeSignatures(mixed) == [s.Serialize() for s in mixed] == [W.compress(1, W.G.unwire(1, x)) for x in (w[0], w[1], None, w[2])]
    w2 = W.G.wire(2, W.G.subgroup_points(2)[0])
    assert g2pubs.NewPublicKeyFromG2Projective(jac2(xs, w2)).Serialize() == W.compress(2, W.G.unwire(2, w2))
