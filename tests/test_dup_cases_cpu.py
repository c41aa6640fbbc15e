"""CPU: the duplicate-rule corpus (dup_cases.py) holds what it claims, and its model is the oracle's VerifyAggregate.

At n = 33, for g2pubs and g1pubs, the aggregate of every case is a correct signature of the messages as they stand (every re-signed
tuple verifies, the unchanged base verifies), so the oracle's verdict is the duplicate rule's alone -- and must equal rule(msgs).  The
corpus' own claims -- positions, lengths, both verdicts in every family, near-equal messages really distinct -- are checked at 33, 4 096
and 4 097 messages, the sizes the GPU tests use."""
from concurrent.futures import ThreadPoolExecutor

import pytest

import dup_cases as D

SIZES = (33, 4096, 4097)
NEAR_EQUAL = ("nul_appended", "prefix", "one_byte_differs", "same_concat", "one_byte_messages", "byte_199")
MUST_FIRE = ("pair_pos", "pair_len", "triple", "two_pairs", "whole_batch", "empty", "empty_and_pair")


def _equal_groups(msgs):
    """{message: its positions} of the messages that occur more than once"""
    at = {}
    for p, m in enumerate(msgs):
        at.setdefault(m, []).append(p)
    return {m: ps for m, ps in at.items() if len(ps) > 1}


@pytest.mark.parametrize("n", SIZES)
def test_corpus_holds_what_it_claims(n):
    base = D.base_messages(n)
    assert len(set(base)) == n and all(base) and D.rule(base) is True
    assert len({len(m) for m in base}) > 8                                 # ragged
    cases = {c.name: c for c in D.corpus(n)}
    msgs = {name: D.apply(base, c) for name, c in cases.items()}
    verdict = {name: D.rule(m) for name, m in msgs.items()}
    fam = {}
    for c in cases.values():
        fam.setdefault(c.family, []).append(c.name)
    assert set(fam) == set(NEAR_EQUAL) | set(MUST_FIRE)
    for f, names in fam.items():                                           # both verdicts in every family
        assert {verdict[k] for k in names} == {True, False}, f
    # equal pairs at the listed positions (those that fit into n), and nothing else equal in those cases
    want = [(0, 1), (0, n - 1), (n - 2, n - 1)] + ([(0, 255), (255, 256)] if n > 256 else [])
    got = []
    for c in D.position_cases(cases.values()):
        groups = _equal_groups(msgs[c.name])
        assert len(groups) == 1 and verdict[c.name] is False
        got.append(tuple(*groups.values()))
    assert sorted(got) == sorted(want)
    # an equal pair of every listed length, and beside it a pair of that length that differs in its last byte
    for length in (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 200):
        (name,) = [k for k in fam["pair_len"] if k.startswith("pair_len%d@" % length)]
        ((m, ps),) = _equal_groups(msgs[name]).items()
        assert len(m) == length and len(ps) == 2 and verdict[name] is False
        (twin,) = [k for k in fam["pair_len"] if k.startswith("pair_len%d_last" % length)]
        a, b = (msgs[twin][p] for p in ps)
        assert len(a) == len(b) == length and a[:-1] == b[:-1] and a != b and verdict[twin] is True
    assert [sorted(map(len, _equal_groups(msgs[k]).values())) for k in ("three_equal", "two_pairs", "all_equal")] == [[3], [2, 2], [n]]
    assert sorted(min(c.changes) for c in D.empty_cases(cases.values())) == [0, n // 2, n - 1]
    for c in D.empty_cases(cases.values()):
        assert msgs[c.name].count(b"") == 1 and not _equal_groups(msgs[c.name]) and verdict[c.name] is False
    m = msgs["empty_and_pair"]
    assert m.count(b"") == 1 and [len(v) for v in _equal_groups(m).values()] == [2] and verdict["empty_and_pair"] is False
    # near-equal messages: the rule accepts, every message is distinct, and the pair is what the name says
    wg = D.WG
    for f in NEAR_EQUAL:
        for name in fam[f]:
            if verdict[name]:
                assert len(set(msgs[name])) == n and all(msgs[name]), name
    for name, c in cases.items():
        if name.endswith(("@same_wg", "@diff_wg")) and len(c.changes) == 2:
            a, b = sorted(c.changes)
            assert (a // wg == b // wg) == (name.endswith("@same_wg") or n <= wg), name
    for length in (7, 8, 15):
        for w in ("same_wg", "diff_wg"):
            a, b = cases["nul_appended_len%d@%s" % (length, w)].changes.values()
            assert len(a) == length and b == a + b"\0" and 0 not in a
    for cut in (13, 16):
        a, b = cases["prefix%d@same_wg" % cut].changes.values()
        assert b == a[:cut] and len(a) > cut
    for what, k in (("first", 0), ("last", 20), ("tail", 17), ("word_end", 15)):
        a, b = cases["%s_byte_differs@diff_wg" % what].changes.values()  # 21 bytes: two words and a tail of bytes 16 .. 20
        assert len(a) == len(b) == 21 and [i for i in range(21) if a[i] != b[i]] == [k]
    for w in ("same_wg", "diff_wg"):
        ch = cases["same_concat@%s" % w].changes
        pos = sorted(ch)
        assert [ch[p] for p in pos] == [b"ab", b"c", b"a", b"bc"] and pos[1] == pos[0] + 1 and pos[3] == pos[2] + 1
        assert (pos[0] // wg == pos[3] // wg) == (w == "same_wg" or n <= wg)
        a, b = cases["byte199_differs@%s" % w].changes.values()
        assert len(a) == len(b) == 200 and [i for i in range(200) if a[i] != b[i]] == [199]
    one = cases["one_byte_messages"].changes
    assert sorted(one.values()) == [bytes([v]) for v in range(min(n, 256))]
    if n > 256:
        assert {p // wg for p in one} == set(range(n // wg))               # in every full work-group
    # what the GPU tests take for the further forms
    assert len(D.position_cases(cases.values())) == len(want) and len(D.empty_cases(cases.values())) == 3
    near = D.near_equal_cases(cases.values())
    assert len(near) == 3 and all(verdict[c.name] for c in near)


@pytest.fixture(scope="module", params=["g2pubs", "g1pubs"])
def signed(request):
    return D.Signed(request.param, 33)


def test_oracle_verdict_is_the_models(signed):
    """the premise (every re-signed tuple verifies; the base verifies) and then the oracle's VerifyAggregate against rule()"""
    o = signed.o
    assert all(o.verify(m, signed.keys[i], s) is True for i, (m, s) in enumerate(zip(signed.msgs, signed.sigs)))
    assert o.verify_aggregate(signed.agg, signed.keys, signed.msgs) is True

    def one(c):
        msgs, agg, _ = signed.case(c)
        return c.name, signed.premise(c), o.verify_aggregate(agg, signed.keys, msgs), D.rule(msgs)
    with ThreadPoolExecutor(8) as ex:                                      # (the oracle's C calls release the interpreter lock)
        rows = list(ex.map(one, signed.cases))
    assert len(rows) == len(D.corpus(33)) > 60
    wrong = [r for r in rows if not (r[1] is True and r[2] is r[3])]
    assert not wrong, wrong
    assert {r[3] for r in rows} == {True, False}


def test_a_prefix_of_a_signed_base_is_a_signed_base(signed):
    """Signed.prefix(n): the first n tuples, nothing signed again -- the 4 096-message set of the GPU tests is cut from the 4 097-message one"""
    sub = D.Signed(signed.group, 40).prefix(33)
    assert sub.msgs == signed.msgs and sub.sigs == signed.sigs and sub.agg == signed.agg and sub.keys == signed.keys
