#!/usr/bin/env python3
"""Search for HashG2WithDomain inputs with a chosen try-and-increment counter (g2.go:1041-1085).

The reference's loop tests x0, x0 + 1, ... until x^3 + b is a square in Fq2; a message stops at counter c with probability 2^-(c+1),
so the counters at which the device forms of the loop change rounds (8, 16, ... for the eight-per-round forms; 64 / open for the
shared-wave form) do not turn up in a test's handful of random messages.  This tool scans the deterministic family

    message(i) = sha256(b"tai-corpus-%d" % i),   domain = bytes(range(1, 9)),   i = 0 .. 2^21 - 1

on the CPU with the big-integer oracle (oracle/pyref.py) and prints, per counter value, the first few indices that have it.
tests/tai_corpus.py holds the committed result; tests/test_tai_corpus_cpu.py recomputes every listed counter.  No test runs this
scan (about 25 CPU-minutes; --workers processes, 16 at the most).

An element of Fq2 is a square iff its norm is a square in Fq (or it is zero), so a candidate costs one norm and one Euler test.

    python tools/tai_search.py                      # the whole family
    python tools/tai_search.py --hi 40000 --keep 4  # a quick look
"""
import argparse
import hashlib
import multiprocessing
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import pyref as P  # noqa: E402

DOMAIN = bytes(range(1, 9))
FAMILY_BITS = 21
CHUNK = 4096


def message(i):
    return hashlib.sha256(b"tai-corpus-%d" % i).digest()


def counter(msg32, domain8=DOMAIN):
    """the number of increments the reference's loop makes before x0 + counter gives a square"""
    x = (int.from_bytes(P._sha(msg32 + domain8 + b"\x01"), "big"), int.from_bytes(P._sha(msg32 + domain8 + b"\x02"), "big"))
    c = 0
    while True:
        gx = P.fq2_add(P.fq2_mul(P.fq2_sqr(x), x), P.B_COEFF_FQ2)
        norm = (gx[0] * gx[0] + gx[1] * gx[1]) % P.Q
        if pow(norm, P.Q_MINUS_1_OVER_2, P.Q) in (0, 1):
            return c
        x = P.fq2_add(x, P.FQ2_ONE)
        c += 1


def _scan(bounds):
    lo, hi = bounds
    return [(i, counter(message(i))) for i in range(lo, hi)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--lo", type=int, default=0)
    ap.add_argument("--hi", type=int, default=1 << FAMILY_BITS)
    ap.add_argument("--keep", type=int, default=8, help="indices printed per counter value")
    ap.add_argument("--workers", type=int, default=16)
    a = ap.parse_args()
    workers = max(1, min(16, a.workers))
    chunks = [(lo, min(lo + CHUNK, a.hi)) for lo in range(a.lo, a.hi, CHUNK)]
    first, count = {}, {}
    with multiprocessing.Pool(workers) as pool:
        for part in pool.imap(_scan, chunks):                               # in order: "the first few" is well defined
            for i, c in part:
                count[c] = count.get(c, 0) + 1
                if len(first.setdefault(c, [])) < a.keep:
                    first[c].append(i)
    print("# messages %d .. %d, domain %s" % (a.lo, a.hi - 1, DOMAIN.hex()))
    print("# counter: how many -- first indices")
    for c in sorted(first):
        print("%2d: %7d -- %s" % (c, count[c], first[c]))
    missing = [c for c in range(max(first) + 1) if c not in first]
    if missing:
        print("# absent below the maximum: %s" % missing)


if __name__ == "__main__":
    main()
