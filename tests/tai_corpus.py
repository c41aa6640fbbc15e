"""HashG2WithDomain inputs with a KNOWN try-and-increment counter (g2.go:1065-1084: the number of x0 += 1 steps before x0^3 + b is a square).

A message stops at counter c with probability 2^-(c+1), so random test messages never reach the later rounds of the device forms of the
loop (hash.cuh: tai_g2_group8 and tai_g2_waves8 test eight candidates a round, tai_g2_wave 64 / open per open message).  The table below
is the result of tools/tai_search.py over

    message(i) = sha256(b"tai-corpus-%d" % i),   domain = bytes(range(1, 9)),   i = 0 .. 2^21 - 1

(counts per value over the 2 097 152 messages: 0: 1 049 543, 1: 523 513, 2: 262 298, 3: 130 596, 4: 65 482, 5: 32 897, 6: 16 488, 7: 8 150,
8: 4 099, 9: 2 081, 10: 1 003, 11: 479, 12: 268, 13: 137, 14: 57, 15: 37, 16: 11, 17: 7, 18: 3, 19: 1, 20: 1, 25: 1; 21 .. 24 did not occur).
It lists the first indices of every value up to 15 and every index from 16 on.  tests/test_tai_corpus_cpu.py recomputes each counter with the
big-integer oracle and proves with wave_schedule() that the named batches reach the states they are meant to; tests/test_gpu_tai_search.py
runs them through every device form.  Nothing here needs a GPU.
"""
import hashlib

DOMAIN = bytes(range(1, 9))

# counter -> indices i of message(i), in increasing order
COUNTERS = {
    0: [2, 3, 5, 7, 8, 11, 12, 14, 15, 16, 19, 20, 21, 23, 24, 25, 26, 31, 33, 35, 36, 38, 40, 41, 43, 45, 48, 51, 54, 55, 56, 58, 60, 61, 62, 65,
        67, 70, 72, 73, 78, 81, 82, 83, 85, 86, 89, 92, 93, 94, 96, 97, 98, 100, 103, 104, 105, 107, 108, 110, 111, 113, 114, 115],
    1: [1, 10, 13, 17, 22, 27],
    2: [0, 6, 28, 30, 57, 75],
    3: [4, 18, 46, 50, 64, 68],
    4: [32, 39, 102, 116, 173, 177],
    5: [9, 37, 44, 149, 292, 310],
    6: [59, 136, 250, 260, 472, 507],
    7: [219, 408, 484, 533, 1046, 1371],
    8: [169, 477, 895, 1136, 1219, 1683],
    9: [965, 3405, 3620, 5224, 6094, 8267],
    10: [5621, 10776, 11458, 12100, 13964, 14374],
    11: [1160, 2681, 6535, 17344, 20790, 29953],
    12: [4733, 12120, 24782, 26648, 34485, 38195],
    13: [9548, 16647, 73438, 73826, 80772, 87536],
    14: [44809, 53141, 83976, 99438, 126292, 150982],
    15: [74088, 86855, 116611, 240370, 284020, 320261],
    16: [178484, 241565, 633435, 976379, 1096725, 1420339, 1504104, 1549163, 1653557, 1692977, 1854320],
    17: [30938, 331378, 345943, 952383, 1371640, 1620589, 1661355],
    18: [1303596, 1757877, 2067019],
    19: [1998851],
    20: [410490],
    25: [698317],
}
MAX_COUNTER = max(COUNTERS)
COUNTER_OF = {i: c for c, idx in COUNTERS.items() for i in idx}


def message(i):
    """the 32-byte message of index i"""
    return hashlib.sha256(b"tai-corpus-%d" % i).digest()


def messages(indices):
    return [message(i) for i in indices]


def indices_with(lo, hi=MAX_COUNTER):
    """every listed index whose counter lies in lo .. hi, by counter, then by index"""
    return [i for c in sorted(COUNTERS) if lo <= c <= hi for i in COUNTERS[c]]


def counters_of(indices):
    return [COUNTER_OF[i] for i in indices]


def waves_of(indices):
    """a call's messages as tai_g2_wave sees them: 64 to a wave, the last one ragged"""
    return [indices[k:k + 64] for k in range(0, len(indices), 64)]


# ---- a model of tai_g2_wave's rounds (hash.cuh, the comment block above it and its while loop) -------------------------------------------
def wave_schedule(counters):
    """The rounds of one wave of tai_g2_wave over messages with these counters (1 .. 64 of them, in lane order).

    A round hands the wave's 64 lanes to the messages still open: k = 64 // open consecutive candidates nextc .. nextc + k - 1 of each, the
    64 - open * k lanes left over idle.  A message closes in the round whose range holds its counter (the smallest passing candidate wins:
    everything below the counter fails by definition); the others move nextc on by k.  Round 0 of a full wave has k = 1, candidate 0.

    Returns a list of rounds, each a dict:
      open    the wave-local indices of the open messages, ascending (the kernel's compacted `list`)
      k       candidates per open message
      idle    lanes without a candidate
      first   {message: the first candidate of its range}; the last one is first + k - 1
      closes  the messages that close in this round, ascending
      own_x0  True where every lane works for its own message (all 64 open: the kernel keeps x0 and skips the two SHA-256 blocks)
    """
    n = len(counters)
    assert 1 <= n <= 64
    nextc = [0] * n
    still = list(range(n))
    rounds = []
    while still:
        k = 64 // len(still)
        closes = [m for m in still if nextc[m] <= counters[m] < nextc[m] + k]
        rounds.append({"open": list(still), "k": k, "idle": 64 - len(still) * k, "first": {m: nextc[m] for m in still},
                       "closes": closes, "own_x0": len(still) == 64})
        still = [m for m in still if m not in closes]
        for m in still:
            nextc[m] += k
    return rounds


def rounds_of_eight(counters):
    """the rounds an eight-candidates-a-round form (tai_g2_group8 per wave of eight messages, tai_g2_waves8 per message) makes until the
    slowest of these messages has closed: round r tests the candidates 8 r .. 8 r + 7"""
    return max(counters) // 8 + 1


# ---- named batches: lists of indices, 64 to a wave; what each must reach is asserted in tests/test_tai_corpus_cpu.py ----------------------
def _c(c, j=0):
    return COUNTERS[c][j]


_ZERO = COUNTERS[0]
_TOP = COUNTERS[MAX_COUNTER][0]


def _wave_with(chosen, lanes=64):
    """a wave of counter-0 messages with `chosen` = {lane: index} in their places"""
    zeros = iter(_ZERO)
    return [chosen[l] if l in chosen else next(zeros) for l in range(lanes)]


def _batch_a():
    # 33 lanes carry the message with the largest counter, so more than 32 stay open -- k = 1 -- up to the last round; the other 31 lanes
    # (the odd ones) carry distinct messages with counters 2 .. 7
    others = [i for c in (2, 3, 4, 5, 6) for i in COUNTERS[c]] + [_c(7)]
    return [others[l // 2] if l % 2 and l // 2 < 31 else _TOP for l in range(64)]


def _batch_a_distinct():
    # 64 different messages with counters >= 2, the largest among them: rounds 1 and 2 with all lanes open, then k grows as they close
    idx = [i for c in range(2, 12) for i in COUNTERS[c]] + [_c(18), _c(19), _c(20), _TOP]
    return idx[7:] + idx[:7]                                               # (the top counters in the middle of the wave)


def _batch_g():
    # eight waves of eight messages: the largest counter at group position w of wave w, around it counters 0, 7, 8, 15, 16, 17, 0;
    # then five more messages, a count that is no multiple of eight
    out = []
    for w in range(8):
        others = [_ZERO[2 * w], _c(7, w % 6), _c(8, w % 6), _c(15, w % 6), _c(16, w), _c(17, w % 7), _ZERO[2 * w + 1]]
        out += others[:w] + [_TOP] + others[w:]
    return out + [_c(16, 8), _ZERO[16], _c(7), _c(15), _c(8)]


BATCHES = {
    # (a) a full wave, every counter >= 2, the corpus maximum in it: rounds 1 and 2 with all 64 lanes open, MAX_COUNTER + 1 rounds in all
    "a": _batch_a(),
    "a_distinct": _batch_a_distinct(),
    # (b) counter-0 messages and nine chosen ones: round 1 open = 9, k = 7 (one lane idle), closes on its first (1) and last (7) candidate;
    # six go on to round 2 with open = 6, k = 10, closes on its first (8) and last (17) candidate; counter 18 goes on alone
    "b": _wave_with({3: _c(1), 9: _c(8), 17: _c(4), 22: _c(17), 31: _c(10), 40: _c(7), 47: _c(18), 58: _c(13), 63: _c(16)}),
    # (c) one message open in round 1: k = 64, candidates 1 .. 64
    "c": _wave_with({41: _c(20)}),
    # (d) three messages open in round 1: k = 21 (one lane idle), candidates 1 .. 21
    "d": _wave_with({0: _c(12), 30: _c(1), 63: _c(19)}),
    # (e) the same message twice in one wave (a wave of ten: k = 6 from round 0)
    "e": [_ZERO[0], _c(8), _ZERO[1], _c(8), _c(2), _ZERO[0], _c(16), _c(3), _c(16), _c(5)],
    # (f) ragged ends: a full wave and a last wave of 1 message (k = 64 from round 0), of 37
    "f1": _wave_with({5: _c(1, 1), 20: _c(3, 1), 50: _c(6, 1)}) + [_c(17)],
    "f37": _wave_with({0: _c(2, 1), 33: _c(9), 63: _c(4, 1)}) + _wave_with({0: _c(14), 7: _c(1, 2), 13: _c(2, 2), 21: _c(9, 1), 29: _c(5, 1), 33: _c(1, 3), 36: _c(2, 3)}, 37),
    # (g) the eight-lane form
    "g": _batch_g(),
}
WAVE_BATCHES = ["a", "a_distinct", "b", "c", "d", "f37", "f1", "e"]      # the order of the one concatenated call (the first five keep their waves)
