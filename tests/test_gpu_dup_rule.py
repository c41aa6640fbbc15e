"""-m gpu: the duplicate-message rule of VerifyAggregate where it alone decides the verdict, on every path that applies it.

The cases come from dup_cases.py: the aggregate of a case is a correct signature of the messages as they stand (the changed positions are
signed again by the oracle), so the pairing equation holds and the expected verdict is the rule's -- dup_cases.rule, the reference's
sort-and-compare (g2pubs/bls.go:245-261), which test_dup_cases_cpu.py holds against the oracle's VerifyAggregate.  A missed duplicate
shows as True where the model says False, a false duplicate as False where it says True.  Every rejected case is run again with its
changed messages put back (same keys, the base aggregate) and must then verify.

  device table (k_util.hip)            n = 4097: the host form and every device-pointer / prepared form
  its fallback, dup_sort_fallback      the same under set_option("dup_force_sort", 1): host messages, and messages fetched from the device
  inline host table, has_duplicates    n = 33 and n = 4096, the last size screened inline; the sort under dup_force_sort
  a host thread beside the shards      dup_rule_worker.py: a split call in a child process, without and with BLSMI_DUP_FORCE_SORT
  WithDomain forms                     no such rule: two equal messages verify"""
import hashlib
import json
import os
import pickle
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import dup_cases as D
from gpu_common import P, RC, g1_to_jac, g2_to_jac, sk_bytes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = ("g2pubs", "g1pubs")
N_DEVICE, N_INLINE, N_SMALL = 4097, 4096, 33                              # DUP_INLINE_MAX = 4096 (verify_host.inc)
FAMILIES = sorted({c.family for c in D.corpus(N_DEVICE)})
NEAR_EQUAL = ("nul_appended", "prefix", "one_byte_differs", "same_concat", "one_byte_messages", "byte_199")
DOMAIN = bytes(range(1, 9))


@pytest.fixture(scope="module")
def eng():
    from bls_amd import engine
    engine.init(0)
    return engine


def _dev(x):
    import torch
    a = np.frombuffer(x, dtype=np.uint8).copy() if isinstance(x, (bytes, bytearray)) else np.array(x)
    if a.dtype in (np.uint64, np.uint32):
        a = a.view(np.int64 if a.dtype == np.uint64 else np.int32)
    return torch.from_numpy(a).to(torch.device("cuda", 0))


@pytest.fixture(scope="module")
def signed():
    """{(group, n): dup_cases.Signed}: 4 097 messages signed once per package by the oracle; the smaller sets are their first n tuples"""
    out = {}
    for g in GROUPS:
        big = D.Signed(g, N_DEVICE)
        out[g, N_DEVICE], out[g, N_INLINE], out[g, N_SMALL] = big, big.prefix(N_INLINE), big.prefix(N_SMALL)
        o = big.o
        for i in (0, 1, N_SMALL - 1, N_INLINE - 1, N_DEVICE - 1):
            assert o.verify(big.msgs[i], big.keys[i], big.sigs[i]) is True
        small = out[g, N_SMALL]
        assert o.verify_aggregate(small.agg, small.keys, small.msgs) is True
    return out


class Forms:
    """the forms of VerifyAggregate over one signed set; the keys are uploaded / converted / prepared once"""

    def __init__(self, eng, s):
        self.eng, self.s, self.n = eng, s, s.n
        self.pk_b = b"".join(s.keys)
        self.d_k = _dev(self.pk_b)
        self.host_fn = eng.g2pubs_verify_aggregate if s.g2 else eng.g1pubs_verify_aggregate
        self._jac = self._tables = self._own = None

    def host(self, msgs, agg):
        return self.host_fn(msgs, self.pk_b, agg)

    def _resident(self, msgs):
        off = np.zeros(len(msgs) + 1, dtype=np.uint64); off[1:] = np.cumsum([len(m) for m in msgs])
        return _dev(b"".join(msgs) or b"\0"), _dev(off)

    def dev(self, msgs, agg):
        d_m, d_o = self._resident(msgs)
        return self.eng.verify_aggregate_dev(self.s.group, d_m.data_ptr(), d_o.data_ptr(), self.d_k.data_ptr(), agg, self.n)

    def jac(self, msgs, agg):
        s = self.s
        if self._jac is None:
            one = [(g2_to_jac if s.g2 else g1_to_jac)(pk) for pk in s.pks]
            self._jac = b"".join(one[i] for i in s.key_idx)
        fn = self.eng.g2pubs_verify_aggregate_jac if s.g2 else self.eng.g1pubs_verify_aggregate_jac
        return fn(msgs, self._jac, (g1_to_jac if s.g2 else g2_to_jac)(agg))

    def prepared(self):
        """g2pubs: {name: form} over prepared keys, with key_idx into the NK signers' tables and without (tuple t uses table t)"""
        eng, s = self.eng, self.s
        if self._tables is None:
            self._tables, self._own = eng.PreparedKeys(b"".join(s.pks), D.NK), eng.PreparedKeys(self.pk_b, self.n)
            self._idx = np.array(s.key_idx, dtype=np.uint32)
            self._d_idx = _dev(self._idx)
        out = {}
        for tag, tab, idx, d_idx in (("[idx]", self._tables, self._idx, self._d_idx.data_ptr()), ("", self._own, None, 0)):
            def host(msgs, agg, tab=tab, idx=idx):
                return eng.g2pubs_verify_aggregate_prepared(msgs, tab, idx, agg)

            def jac(msgs, agg, tab=tab, idx=idx):
                return eng.g2pubs_verify_aggregate_prepared_jac(msgs, tab, idx, g1_to_jac(agg))

            def dev(msgs, agg, tab=tab, d_idx=d_idx):
                d_m, d_o = self._resident(msgs)
                return eng.g2pubs_verify_aggregate_prepared_dev(d_m.data_ptr(), d_o.data_ptr(), tab.ptr, d_idx, agg, self.n)
            out.update({"prepared" + tag: host, "prepared_jac" + tag: jac, "prepared_dev" + tag: dev})
        return out

    def close(self):
        for t in (self._tables, self._own):
            if t is not None:
                t.close()


@pytest.fixture(scope="module")
def forms(eng, signed):
    out = {k: Forms(eng, s) for k, s in signed.items()}
    yield out
    for f in out.values():
        f.close()


def _check(s, named_forms, cases):
    """Every case through every form: the model's verdict; a rejected case verifies once its changed messages are put back.  Returns the
    number of (case, form) runs."""
    assert cases and named_forms
    wrong, ran = [], 0
    for c in cases:
        msgs, agg, _ = s.case(c)
        assert s.premise(c), c.name                                        # every re-signed tuple is a valid signature: the rule alone decides
        want = D.rule(msgs)
        back = list(msgs)
        for p in c.changes:
            back[p] = s.msgs[p]
        assert back == s.msgs
        for fname, form in named_forms.items():
            got = form(msgs, agg)
            restored = form(back, s.agg) if not want else True
            ran += 1
            if got is not want or restored is not True:
                wrong.append((s.group, s.n, c.name, fname, "model", want, "got", got, "restored", restored))
    assert not wrong, wrong
    return ran


def _family(s, family):
    return [c for c in s.cases if c.family == family]


def _further(s):
    cases = list(s.cases)
    return D.position_cases(cases) + D.empty_cases(cases) + D.near_equal_cases(cases)


class forced_sort:
    """set_option("dup_force_sort", 1) for the block: every screen takes its fallback, the reference's sort"""

    def __init__(self, eng, on=True):
        self.eng, self.on = eng, on

    def __enter__(self):
        if self.on:
            self.eng.set_option("dup_force_sort", 1)

    def __exit__(self, *exc):
        self.eng.set_option("dup_force_sort", 0)


@pytest.mark.parametrize("forced", [False, True], ids=["table", "forced_sort"])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("group", GROUPS)
def test_device_screen_whole_corpus_host_and_dev_forms(eng, signed, forms, group, family, forced):
    """n = 4097: the host form stages its messages and screens them on the device, the _dev form's are resident.  forced_sort:
    dup_sort_fallback, reading the host's messages for the one and fetching them back from the device for the other."""
    s, f = signed[group, N_DEVICE], forms[group, N_DEVICE]
    cases = _family(s, family)
    assert {D.rule(s.case(c)[0]) for c in cases} == {True, False}
    with forced_sort(eng, forced):
        assert _check(s, {"host": f.host, "dev": f.dev}, cases) == 2 * len(cases)


@pytest.mark.parametrize("group", GROUPS)
def test_device_screen_further_forms(eng, signed, forms, group):
    """n = 4097, the position cases, the empty cases and three near-equal cases: in-memory points, and for g2pubs the prepared forms
    (host, in-memory signature, resident), with key_idx and with one table per tuple"""
    s, f = signed[group, N_DEVICE], forms[group, N_DEVICE]
    cases = _further(s)
    assert len(cases) == 5 + 3 + 3
    named = {"jac": f.jac}
    if s.g2:
        named.update(f.prepared())
    assert len(named) == (7 if s.g2 else 1)
    assert _check(s, named, cases) == len(named) * len(cases)


@pytest.mark.parametrize("forced", [False, True], ids=["table", "forced_sort"])
@pytest.mark.parametrize("group", GROUPS)
def test_inline_host_screen_whole_corpus_at_33(eng, signed, forms, group, forced):
    """n = 33: has_duplicates on the calling thread (forced_sort: has_duplicates_sorted), no device screen"""
    s, f = signed[group, N_SMALL], forms[group, N_SMALL]
    with forced_sort(eng, forced):
        assert _check(s, {"host": f.host}, list(s.cases)) == len(s.cases)


@pytest.mark.parametrize("forced", [False, True], ids=["table", "forced_sort"])
@pytest.mark.parametrize("group", GROUPS)
def test_device_screen_of_the_dev_form_at_33(eng, signed, forms, group, forced):
    """the _dev form screens on the device at any size: a table of 1 024 slots, one work-group"""
    s, f = signed[group, N_SMALL], forms[group, N_SMALL]
    with forced_sort(eng, forced):
        assert _check(s, {"dev": f.dev}, _further(s)) == len(_further(s))


@pytest.mark.parametrize("forced", [False, True], ids=["table", "forced_sort"])
@pytest.mark.parametrize("group", GROUPS)
def test_inline_host_screen_at_4096_agrees_with_the_device_screen_at_4097(eng, signed, forms, group, forced):
    """4 096 messages are the most the host form screens inline; one more and the device does.  The position and the near-equal cases,
    the same case (by its place in the corpus) at both sizes: the model's verdict at each, hence the same"""
    s0, s1 = signed[group, N_INLINE], signed[group, N_DEVICE]
    pick = [i for i, c in enumerate(s0.cases) if c.family in NEAR_EQUAL or D.is_position_case(c)]
    assert len(pick) == 5 + sum(c.family in NEAR_EQUAL for c in s0.cases) > 30
    with forced_sort(eng, forced):
        for i in pick:
            c0, c1 = s0.cases[i], s1.cases[i]
            assert (c0.family, c0.name.split("@")[0]) == (c1.family, c1.name.split("@")[0])
            assert D.rule(s0.case(c0)[0]) is D.rule(s1.case(c1)[0])
        assert _check(s0, {"host": forms[group, N_INLINE].host}, [s0.cases[i] for i in pick]) == len(pick)
        assert _check(s1, {"host": forms[group, N_DEVICE].host}, [s1.cases[i] for i in pick]) == len(pick)


def _split_call_data(s):
    """plain data for dup_rule_worker.py: the position cases, one empty case and two near-equal cases, signed and checked here"""
    cases = list(s.cases)
    cases = D.position_cases(cases) + D.empty_cases(cases)[1:2] + D.near_equal_cases(cases)[:2]
    rows = []
    for c in cases:
        msgs, agg, _ = s.case(c)
        assert s.premise(c), c.name
        rows.append({"name": c.name, "changes": dict(c.changes), "agg": agg, "model": D.rule(msgs)})
    return {"keys": b"".join(s.keys), "msgs": list(s.msgs), "agg": s.agg, "cases": rows}


@pytest.mark.parametrize("forced", [False, True], ids=["table", "forced_sort"])
def test_split_call_host_thread_beside_the_shards(signed, tmp_path, forced):
    """A split call (BLSMI_SHARDS=2) screens on a host thread beside the shards (verify_aggregate_host: dup_thread), with the keyed table
    and, with BLSMI_DUP_FORCE_SORT in the child's environment, the sort.  One fresh child process each: both are read at start-up."""
    sets = tmp_path / "split_call.pickle"
    with open(sets, "wb") as fh:
        pickle.dump({g: _split_call_data(signed[g, N_DEVICE]) for g in GROUPS}, fh)
    env = dict(os.environ)
    env.update({"BLSMI_SHARDS": "2", "BLSMI_SHARD_MIN": "64"})
    env.pop("BLSMI_DUP_FORCE_SORT", None)
    if forced:
        env["BLSMI_DUP_FORCE_SORT"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "dup_rule_worker.py"), str(sets)], env=env, capture_output=True, text=True, timeout=300)
    line = [l for l in r.stdout.splitlines() if l.startswith("DUP_RULE_RESULT ")]
    assert r.returncode == 0 and line, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    res = json.loads(line[-1][len("DUP_RULE_RESULT "):])
    assert res["shards"] == 2 and res["forced"] is forced, res
    for g in GROUPS:
        rows = res["runs"][g]
        assert len(rows) == 5 + 1 + 2
        wrong = [row for row in rows if row["got"] is not row["model"] or row["restored"] is not True]
        assert not wrong, (g, wrong)
        assert {row["model"] for row in rows} == {True, False}
        pairs = [row["shards_of_changed"] for row in rows if row["name"].startswith("pair@")]
        assert [0, 0] in pairs and [1, 1] in pairs and [0, 1] in pairs      # the equal pair in one shard, in the other, and across the two


def test_with_domain_forms_have_no_duplicate_rule(eng):
    """VerifyAggregateWithDomain (g1pubs/bls.go:300-311) does not look for equal messages: 4 097 32-byte messages, three of them equal and
    signed by three keys, verify through the host, in-memory and resident forms -- on the very path that screens the plain forms on the
    device.  The first 33 tuples hold two of the equal messages: the oracle's verdict on them is True as well."""
    n, o = N_DEVICE, RC.g1pubs
    xs = P.XORShift(4097 * 3)
    sks = [sk_bytes(xs) for _ in range(D.NK)]
    pks = [o.priv_to_pub(sk) for sk in sks]
    msgs = [hashlib.sha256(b"with domain %d" % i).digest() for i in range(n)]
    msgs[20] = msgs[n - 1] = msgs[3]
    assert len(set(msgs)) == n - 2 and D.rule(msgs) is False and D.rule(msgs[:N_SMALL]) is False
    todo = list(dict.fromkeys((i % D.NK, m) for i, m in enumerate(msgs)))
    with ThreadPoolExecutor(8) as ex:                                      # (the oracle's C calls release the interpreter lock)
        made = dict(zip(todo, ex.map(lambda t: o.sign_with_domain(t[1], sks[t[0]], DOMAIN), todo)))
    sigs = [made[i % D.NK, m] for i, m in enumerate(msgs)]
    keys = [pks[i % D.NK] for i in range(n)]
    for i in (0, 3, 20, n - 1):
        assert o.verify_with_domain(msgs[i], keys[i], sigs[i], DOMAIN) is True
    assert len({keys[3], keys[20], keys[n - 1]}) == 3
    small = RC.g2_sum(b"".join(sigs[:N_SMALL]), N_SMALL)
    assert o.verify_aggregate_with_domain(small, keys[:N_SMALL], msgs[:N_SMALL], DOMAIN) is True
    agg, pk_b = RC.g2_sum(b"".join(sigs), n), b"".join(keys)
    one = [g1_to_jac(pk) for pk in pks]
    d_m, d_d, d_k = _dev(b"".join(msgs)), _dev(DOMAIN), _dev(pk_b)
    got = {"with_domain": eng.g1pubs_verify_aggregate_with_domain(msgs, DOMAIN, pk_b, agg),
           "with_domain_jac": eng.g1pubs_verify_aggregate_with_domain_jac(msgs, DOMAIN, b"".join(one[i % D.NK] for i in range(n)), g2_to_jac(agg)),
           "with_domain_dev": eng.verify_aggregate_with_domain_dev(d_m.data_ptr(), d_d.data_ptr(), d_k.data_ptr(), agg, n)}
    assert got == {"with_domain": True, "with_domain_jac": True, "with_domain_dev": True}
    other = RC.g2_sum(b"".join(sigs[:n - 1]), n - 1)                       # (and the verdict is the equation's: another aggregate fails)
    assert eng.g1pubs_verify_aggregate_with_domain(msgs, DOMAIN, pk_b, other) is False
