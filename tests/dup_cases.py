"""Message sets for the duplicate-message rule of VerifyAggregate (g2pubs/bls.go:245-261, g1pubs/bls.go:257-273), with the rule as a model.

corpus(n) gives named cases over a base of n distinct ragged messages; a case changes a handful of positions.  rule(msgs) is the
reference's sort-and-compare in plain Python: False iff a message is empty or two are equal.  Every family holds cases the rule
rejects and cases it accepts: an equal pair and, at the same positions, a pair that differs in one byte; an empty message and the
one-byte message b"\\0" in its place; x beside x + b"\\0" and, as their twin, the same message twice.

Signed(group, n) signs the base once with the oracle and, per case, re-signs only the changed positions and sums again, so the aggregate
is the correct signature of the messages as they stand: the pairing equation holds by linearity and the rule alone decides the verdict.
Used by test_dup_cases_cpu.py (the oracle against the model), test_gpu_dup_rule.py and dup_rule_worker.py (the library against the model)."""
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

WG = 256                                                                   # work-group size of k_msg_fingerprint and k_dup_insert
PAIR_LENGTHS = (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 200)                   # around the fingerprint's 8-byte word loop and its tail
NUL_LENGTHS = (7, 8, 15)
NK = 16                                                                    # signers; position i is signed by key i % NK

Case = namedtuple("Case", "name family changes")                           # changes: {position: message}


def rule(msgs):
    """the reference's verdict on the messages alone: sort, compare neighbours, the first against nil (an empty message equals nil)"""
    s = sorted(msgs)
    return all(len(m) > 0 for m in s) and all(s[i] != s[i + 1] for i in range(len(s) - 1))


def base_messages(n):
    """n distinct messages of ragged length (7 .. 60 bytes); every one starts with b"base", which no changed message does"""
    return [(b"base %d " % i) * (1 + i % 4) + bytes(i % 5) for i in range(n)]


def x(length, tag=0):
    """a fixed message of `length` non-zero bytes, first byte 0x80 | tag"""
    return bytes([0x80 | tag] + [(37 * k + 11 * tag) % 251 + 1 for k in range(1, length)])


def flip(m, k):
    return m[:k] + bytes([m[k] ^ 1]) + m[k + 1:]


def pair_positions(n):
    """the issue's positions of an equal pair; (0, 255) and (255, 256) need more than one work-group"""
    want = [(0, 1), (0, WG - 1), (WG - 1, WG), (0, n - 1), (n - 2, n - 1)]
    return [p for p in dict.fromkeys(want) if p[0] < p[1] < n]


def placements(n):
    """where two near-equal messages go: in one work-group, and in two (the second is then the last message: alone in its work-group at
    n = 4097).  A batch of one work-group still gets two placements."""
    if n > 2 * WG:
        return {"same_wg": (3, 200), "diff_wg": (100, n - 1)}
    return {"same_wg": (3, n // 2), "diff_wg": (1, n - 1)}


def corpus(n):
    assert n >= 33
    cases = []

    def add(name, family, changes):
        assert all(0 <= p < n for p in changes)
        cases.append(Case(name, family, dict(changes)))
    where = placements(n)
    spots = list(where.items())
    m24 = x(24, 1)
    # --- families the issue lists under "must fire", each with a twin the rule accepts
    for a, b in pair_positions(n):
        add("pair@%d,%d" % (a, b), "pair_pos", {a: m24, b: m24})
    a, b = pair_positions(n)[-1]
    add("pair_pos_last_byte_differs@%d,%d" % (a, b), "pair_pos", {a: m24, b: flip(m24, 23)})
    for k, length in enumerate(PAIR_LENGTHS):
        wname, (a, b) = spots[k % 2]
        m = x(length, 2)
        add("pair_len%d@%s" % (length, wname), "pair_len", {a: m, b: m})
        add("pair_len%d_last_byte_differs@%s" % (length, wname), "pair_len", {a: m, b: flip(m, length - 1)})
    t = (5, n // 2 + 4, n - 1)
    add("three_equal", "triple", {p: m24 for p in t})
    add("three_nul_padded", "triple", {t[0]: m24, t[1]: m24 + b"\0", t[2]: m24 + b"\0\0"})
    q = ((2, 3), (n - 4, n - 2))
    add("two_pairs", "two_pairs", {q[0][0]: m24, q[0][1]: m24, q[1][0]: x(9, 3), q[1][1]: x(9, 3)})
    add("two_near_pairs", "two_pairs", {q[0][0]: m24, q[0][1]: flip(m24, 0), q[1][0]: x(9, 3), q[1][1]: x(9, 3)[:8]})
    add("all_equal", "whole_batch", {p: m24 for p in range(n)})
    add("base", "whole_batch", {})
    for p in (0, n // 2, n - 1):
        add("empty@%d" % p, "empty", {p: b""})
        add("nul_byte@%d" % p, "empty", {p: b"\0"})
    add("empty_and_pair", "empty_and_pair", {7: b"", 9: m24, n - 1: m24})
    add("nul_byte_and_near_pair", "empty_and_pair", {7: b"\0", 9: m24, n - 1: m24 + b"\0"})
    # --- families the issue lists under "must not fire", in one work-group and in two, each with a twin the rule rejects
    for length in NUL_LENGTHS:                                             # equal tail words, only the length differs
        m = x(length, 4)
        for wname, (a, b) in spots:
            add("nul_appended_len%d@%s" % (length, wname), "nul_appended", {a: m, b: m + b"\0"})
    a, b = where["same_wg"]
    add("nul_appended_twice", "nul_appended", {a: x(7, 4) + b"\0", b: x(7, 4) + b"\0"})
    m20 = x(20, 5)
    for cut in (13, 16):                                                   # a proper prefix, cut inside a word and at a word's end
        for wname, (a, b) in spots:
            add("prefix%d@%s" % (cut, wname), "prefix", {a: m20, b: m20[:cut]})
    a, b = where["diff_wg"]
    add("prefix_twice", "prefix", {a: m20[:13], b: m20[:13]})
    m21 = x(21, 6)                                                         # two words and a tail of five bytes
    for what, k in (("first", 0), ("last", 20), ("tail", 17), ("word_end", 15)):
        for wname, (a, b) in spots:
            add("%s_byte_differs@%s" % (what, wname), "one_byte_differs", {a: m21, b: flip(m21, k)})
    a, b = where["same_wg"]
    add("no_byte_differs", "one_byte_differs", {a: m21, b: m21})
    far = where["diff_wg"][1] - 1
    for wname, p in (("same_wg", 20), ("diff_wg", far - 1)):               # the same concatenated bytes, cut at another offset
        add("same_concat@%s" % wname, "same_concat", {10: b"ab", 11: b"c", p: b"a", p + 1: b"bc"})
    add("same_concat_same_cut", "same_concat", {10: b"ab", 11: b"c", far - 1: b"ab", far: b"c"})
    k = min(n, 256)
    at = [i * (n // k) for i in range(k)]                                  # spread over every work-group
    add("one_byte_messages", "one_byte_messages", {p: bytes([v]) for v, p in enumerate(at)})
    add("one_byte_messages_one_twice", "one_byte_messages", {p: bytes([v if v != k - 1 else 7]) for v, p in enumerate(at)})
    m200 = x(200, 7)
    for wname, (a, b) in spots:
        add("byte199_differs@%s" % wname, "byte_199", {a: m200, b: flip(m200, 199)})
    a, b = where["diff_wg"]
    add("byte199_equal", "byte_199", {a: m200, b: m200})
    assert len({c.name for c in cases}) == len(cases)
    return cases


# what the GPU tests run through the further forms and the split call
def is_position_case(c):
    return c.family == "pair_pos" and c.name.startswith("pair@")


def position_cases(cases):
    return [c for c in cases if is_position_case(c)]


def empty_cases(cases):
    return [c for c in cases if c.name.startswith("empty@")]


def near_equal_cases(cases):
    """three near-equal cases: only the length differs; only the last byte differs; the same concatenation cut elsewhere"""
    return [c for c in cases if c.name in ("nul_appended_len8@diff_wg", "last_byte_differs@same_wg", "same_concat@diff_wg")]


def apply(base, case):
    msgs = list(base)
    for p, m in case.changes.items():
        msgs[p] = m
    return msgs


class Signed:
    """The base of n messages signed once by the oracle (group: "g2pubs" or "g1pubs"), NK keys in rotation; case(c) re-signs what c changes."""

    def __init__(self, group, n, seed=20245, longer=None):
        from gpu_common import P, RC, sk_bytes
        self.group, self.n, self.g2 = group, n, group == "g2pubs"
        self.o = RC.g2pubs if self.g2 else RC.g1pubs
        self._sum = RC.g1_sum if self.g2 else RC.g2_sum
        self.msgs = base_messages(n)
        if longer is None:
            xs = P.XORShift(seed + (0 if self.g2 else 1))
            self.sks = [sk_bytes(xs) for _ in range(NK)]
            self.pks = [self.o.priv_to_pub(sk) for sk in self.sks]
            self.sigs = self._sign(range(n), self.msgs)
        else:                                                              # the first n tuples of a longer base: nothing to sign
            assert longer.group == group and longer.msgs[:n] == self.msgs
            self.sks, self.pks, self.sigs = longer.sks, longer.pks, longer.sigs[:n]
        self.agg = self._sum(b"".join(self.sigs), n)
        self.keys = [self.pks[i % NK] for i in range(n)]
        self.key_idx = [i % NK for i in range(n)]
        self.cases = corpus(n)
        self._memo, self._premise = {}, {}

    def _sign(self, positions, msgs):
        """sign msgs[k] with the key of positions[k]; equal (key, message) pairs are signed once (the oracle's C calls release the
        interpreter lock)"""
        todo = list(dict.fromkeys((p % NK, m) for p, m in zip(positions, msgs)))
        with ThreadPoolExecutor(8) as ex:
            made = dict(zip(todo, ex.map(lambda t: self.o.sign(t[1], self.sks[t[0]]), todo)))
        return [made[(p % NK, m)] for p, m in zip(positions, msgs)]

    def case(self, c):
        """(messages, aggregate signature, the re-signed (position, message, signature) tuples) of a case"""
        if c.name not in self._memo:
            pos = sorted(c.changes)
            new = self._sign(pos, [c.changes[p] for p in pos])
            sigs = list(self.sigs)
            for p, s in zip(pos, new):
                sigs[p] = s
            self._memo[c.name] = (apply(self.msgs, c), self._sum(b"".join(sigs), self.n), [(p, c.changes[p], s) for p, s in zip(pos, new)])
        return self._memo[c.name]

    def premise(self, c):
        """every re-signed tuple is a valid signature by its position's key (at most one per key and message is checked)"""
        if c.name not in self._premise:
            seen = {}
            for p, m, s in self.case(c)[2]:
                seen.setdefault((p % NK, m), s)
            with ThreadPoolExecutor(8) as ex:
                self._premise[c.name] = all(ex.map(lambda t: self.o.verify(t[0][1], self.pks[t[0][0]], t[1]) is True, list(seen.items())))
        return self._premise[c.name]

    def prefix(self, n):
        """the same keys over the first n messages of this base, as a set of its own"""
        return Signed(self.group, n, longer=self)
