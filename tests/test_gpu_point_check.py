"""-m gpu: batch point validation (blsmi 0.14), record for record against oracle.pyref on the corpus of tests/point_check_cases.py: subgroup
points, curve points outside the subgroup, points off the curve, every form of infinity and a coordinate that is not below q, as affine
records and as in-memory Jacobian records under several Z, through the host forms and the device-pointer forms, with check = 0, 1 and 2;
ragged sizes with the status buffer inside a poisoned one; G2 in both lane forms (the one-lane form in one fresh child process under
BLSMI_LAYOUT=single: this file is its own worker); the Python mirrors; and the decompression kernels' err 4 beside the new status 4.

The tests send bad POINTS, never bad buffers: every record is full size and in bounds."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":                                                   # the child process of test_g2_one_lane_form_...: python tests/<this file>
    sys.path.insert(0, ROOT)

import point_check_cases as K
from gpu_common import P

pytestmark = pytest.mark.gpu

GROUPS = (1, 2)
NAME = {1: "g1", 2: "g2"}
CHECKS = (1, 2, 0)
POISON = 0xA5
PAD = 64
CHILD_LIMIT_S = 120
LAT_DEFAULT = 8192


@pytest.fixture(scope="module")
def eng():
    from bls_amd import engine
    engine.init(0)
    return engine


def _dev(b):
    import torch
    a = np.ascontiguousarray(b) if isinstance(b, np.ndarray) else np.frombuffer(bytes(b), dtype=np.uint8)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(torch.device("cuda", 0))


def _host(eng, group, form, cs, check):
    if form == "affine":
        pts, inf = K.affine_buffers(group, cs)
        return (eng.g1_check_batch if group == 1 else eng.g2_check_batch)(pts, len(cs), inf, check)
    return (eng.g1_check_batch_jac if group == 1 else eng.g2_check_batch_jac)(K.jacobian_buffer(cs), len(cs), check)


def _resident(eng, group, form, cs, check):
    """the _dev form: -> (statuses, the PAD bytes before them, the PAD bytes after them, inputs unchanged?)"""
    import torch
    n = len(cs)
    if form == "affine":
        pts, inf = K.affine_buffers(group, cs)
        d_pts, d_inf = _dev(pts), _dev(inf)
    else:
        pts, inf = K.jacobian_buffer(cs), None
        d_pts, d_inf = _dev(pts), None
    d_status = torch.full((n + 2 * PAD,), POISON, dtype=torch.uint8, device=torch.device("cuda", 0))
    eng.check_batch_dev(NAME[group], d_pts.data_ptr(), d_inf.data_ptr() if d_inf is not None else 0, n, d_status.data_ptr() + PAD, jac=form != "affine", check=check)
    torch.cuda.synchronize()
    st = d_status.cpu().numpy()
    same = d_pts.cpu().numpy().tobytes() == bytes(pts) and (d_inf is None or d_inf.cpu().numpy().tobytes() == inf.tobytes())
    return st[PAD:PAD + n].copy(), st[:PAD], st[PAD + n:], same


def _diff(cs, got, want):
    return [(i, cs[i].label, cs[i].src, int(got[i]), int(want[i])) for i in range(len(cs)) if got[i] != want[i]][:8]


@pytest.mark.parametrize("form", ("affine", "jacobian"))
@pytest.mark.parametrize("group", GROUPS)
def test_whole_corpus_host_and_resident_forms_every_check(eng, group, form):
    cs = K.cases(group, form)
    got = {}
    for check in CHECKS:
        want = K.statuses(cs, check)
        h = _host(eng, group, form, cs, check)
        assert h.dtype == np.uint8 and not _diff(cs, h, want), (NAME[group], form, "host", check, _diff(cs, h, want))
        d, before, after, same = _resident(eng, group, form, cs, check)
        assert not _diff(cs, d, want), (NAME[group], form, "resident", check, _diff(cs, d, want))
        assert same, "the _dev form wrote to its inputs"
        assert (before == POISON).all() and (after == POISON).all()
        got[check] = h
    assert (got[1] == got[2]).all()                                            # the endomorphism test and r * P agree record for record
    four = K.statuses(cs, 1) == K.NOT_IN_SUBGROUP
    assert four.any() and (got[0][four] == K.OK).all() and (got[0][~four] == got[1][~four]).all()   # check 0: status 4 becomes 0, nothing else moves


@pytest.mark.parametrize("n", K.SIZES)
@pytest.mark.parametrize("group", GROUPS)
def test_ragged_sizes_inside_a_poisoned_buffer(eng, group, n):
    for form in ("affine", "jacobian"):
        cs = K.cut(K.cases(group, form), n)
        want = K.statuses(cs, 1)
        assert want[-1] != K.OK and (n < 4 or set(want.tolist()) == set(K.STATUSES))
        d, before, after, same = _resident(eng, group, form, cs, 1)
        assert not _diff(cs, d, want), (NAME[group], form, n, _diff(cs, d, want))
        assert (before == POISON).all() and (after == POISON).all(), (NAME[group], form, n, "bytes beyond n were written")
        assert same
        h = _host(eng, group, form, cs, 1)
        assert h.shape == (n,) and not _diff(cs, h, want), (NAME[group], form, n, "host", _diff(cs, h, want))


# ---- G2: the lane-pair form (default) and the one-lane form (BLSMI_LAYOUT=single) ------------------------------------------------------------
def _g2_everything(eng):
    """every G2 status of the corpus and of the ragged cuts, and the kernel names the calls' profiles carry"""
    lib = eng._lib()
    lib.blsmi_set_profiling(1)
    buf = ctypes.create_string_buffer(1 << 14)
    out, names = {}, set()
    try:
        for form in ("affine", "jacobian"):
            cs = K.cases(2, form)
            for check in CHECKS:
                out["%s/%d" % (form, check)] = _host(eng, 2, form, cs, check).tolist()
                lib.blsmi_last_profile(buf, ctypes.c_size_t(len(buf)))
                names |= {item.rsplit("=", 1)[0].strip() for item in buf.value.decode().split(";") if item}
            for n in K.SIZES:
                out["%s/n%d" % (form, n)] = _host(eng, 2, form, K.cut(cs, n), 1).tolist()
    finally:
        lib.blsmi_set_profiling(0)
    return out, sorted(names)


def test_g2_one_lane_form_gives_the_lane_pair_forms_statuses(eng):
    mine, names = _g2_everything(eng)
    assert "k_g2_check_pair" in names and "k_g2_check_jac_pair" in names and "k_g2_check" not in names and "k_g2_check_jac" not in names, names
    env = dict(os.environ, BLSMI_LAYOUT="single")
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    child = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=CHILD_LIMIT_S)   # a new process, never exec
    assert child.returncode == 0, (child.returncode, child.stderr[-2000:])
    theirs = json.loads(child.stdout.strip().splitlines()[-1])
    assert "k_g2_check" in theirs["names"] and "k_g2_check_jac" in theirs["names"], theirs["names"]
    assert not [k for k in theirs["names"] if k.endswith("_pair")], theirs["names"]
    assert theirs["status"].keys() == mine.keys()
    for key in mine:
        assert theirs["status"][key] == mine[key], key
    for form in ("affine", "jacobian"):                                        # (and both are the oracle's)
        assert mine["%s/1" % form] == K.statuses(K.cases(2, form), 1).tolist()


# ---- the Python mirrors ------------------------------------------------------------------------------------------------------------------
def _mixed_points(group, make_wire, make_jac):
    """objects of one group, alternately held in wire form and in in-memory form, and the oracle's statuses"""
    objs, want = [], []
    aff = [c for c in K.affine_cases(group) if not c.inf and any(c.rec)]
    jac = K.jacobian_cases(group)
    for i in range(48):
        if i % 2:
            c = aff[(5 * i) % len(aff)]
            objs.append(make_wire(c.rec))
        else:
            c = jac[(11 * i) % len(jac)]
            objs.append(make_jac(c.rec.tobytes()))
        want.append(c.status)
    c = next(c for c in jac if c.src == "infinity")                            # a Z = 0 record with non-zero X and Y
    objs.append(make_jac(c.rec.tobytes())); want.append(c.status)
    return objs, want


def test_validate_mirrors_on_mixed_lists(eng):
    from bls_amd import g1pubs, g2pubs
    for pkg, pk_group, sig_group in ((g2pubs, 2, 1), (g1pubs, 1, 2)):
        wire_pk = pkg.NewPublicKeyFromG2 if pk_group == 2 else pkg.NewPublicKeyFromG1
        jac_pk = pkg.NewPublicKeyFromG2Projective if pk_group == 2 else pkg.NewPublicKeyFromG1Projective
        wire_sg = pkg.NewSignatureFromG1 if sig_group == 1 else pkg.NewSignatureFromG2
        jac_sg = pkg.NewSignatureFromG1Projective if sig_group == 1 else pkg.NewSignatureFromG2Projective
        pubs, want = _mixed_points(pk_group, wire_pk, jac_pk)
        assert set(want) == set(K.STATUSES)
        assert pkg.ValidatePublicKeys(pubs) == [st in (K.OK, K.INFINITY) for st in want], pkg.__name__
        sigs, swant = _mixed_points(sig_group, wire_sg, jac_sg)
        assert set(swant) == set(K.STATUSES)
        assert pkg.ValidateSignatures(sigs) == [st in (K.OK, K.INFINITY) for st in swant], pkg.__name__
        wire_only = [(p, st) for i, (p, st) in enumerate(zip(pubs[:48], want[:48])) if i % 2]     # one form only: the affine entry point
        assert pkg.ValidatePublicKeys([p for p, _ in wire_only]) == [st in (K.OK, K.INFINITY) for _, st in wire_only]
        assert pkg.ValidatePublicKeys([pkg.NewAggregatePubkey()]) == [True]     # infinity: true, as in the reference


# ---- the decompression kernels' predicate, undisturbed -----------------------------------------------------------------------------------
@pytest.mark.parametrize("group", GROUPS)
def test_decompression_reports_err_4_exactly_where_the_check_reports_4(eng, group):
    cs = [c for c in K.affine_cases(group) if c.status in (K.OK, K.NOT_IN_SUBGROUP) and c.src != "noncanonical"]
    assert sum(1 for c in cs if c.status == K.NOT_IN_SUBGROUP) >= 8 and sum(1 for c in cs if c.status == K.OK) >= 8
    comp = b"".join((P.g1_compress if group == 1 else P.g2_compress)(c.point) for c in cs)
    out, inf, err = (eng.g1_decompress_batch if group == 1 else eng.g2_decompress_batch)(comp, len(cs), 1)
    st = _host(eng, group, "affine", cs, 1)
    assert ((err == 4) == (st == K.NOT_IN_SUBGROUP)).all() and set(err.tolist()) == {0, 4}
    assert all(out[i].tobytes() == cs[i].rec for i in range(len(cs)) if err[i] == 0)
    _, _, err2 = (eng.g1_decompress_batch if group == 1 else eng.g2_decompress_batch)(comp, len(cs), 2)
    assert (err2 == err).all()
    eng.set_latency_threshold(0)                                               # check 1 inside the decompression kernel, not as a level program
    try:
        _, _, err1 = (eng.g1_decompress_batch if group == 1 else eng.g2_decompress_batch)(comp, len(cs), 1)
    finally:
        eng.set_latency_threshold(LAT_DEFAULT)
    assert (err1 == err).all()


if __name__ == "__main__":
    from bls_amd import engine
    engine.init(0)
    status, names = _g2_everything(engine)
    print(json.dumps({"status": status, "names": names}))
