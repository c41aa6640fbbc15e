#!/usr/bin/env python3
"""Grouped randomised batch verification against the plain forms -> profiles/r08_rlc_grouped.log.

One MI355X, host buffers, median of 10 calls, the legs of a shape interleaved:
  a  blsmi_g?pubs_verify_batch_rlc_grouped over a table of d messages
  b  blsmi_g?pubs_verify_batch_rlc on the same tuples with the messages expanded, "rlc_min" = 0
  c  blsmi_g?pubs_verify_batch on the same
Shapes: n in {1 024, 4 096, 16 384, 65 536} x d in {1, 64, n/8, n}, g2pubs and g1pubs; then one bad tuple at the largest n x 64.
b and c are compared on a build of the PARENT commit, in two runs on the same machine, one after the other:
  BLSMI_LIB=<parent build> tools/rlc_grouped_bench.py --only bc --out parent.log      (that library has no leg a)
  tools/rlc_grouped_bench.py --parent parent.log                                       (a, b, c on this build + the parent's b, c per shape)
The second run writes the table with the ratios parent b / a and parent c / a, and states the speed-up at the largest n x 64, where
the grouped form stops paying as d approaches n, and the cost of one bad tuple.

usage: tools/rlc_grouped_bench.py [--only a|bc|abc] [--parent FILE] [--reps 10] [--sizes 1024,4096] [--out profiles/r08_rlc_grouped.log]
"""
import argparse
import hashlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def batch(eng, kind, n, d):
    sks = b"".join(hashlib.sha256(b"bench-sk-%d" % i).digest()[:31].rjust(32, b"\0") for i in range(n))
    table = [b"bench message %d" % j for j in range(d)]
    idx = np.arange(n, dtype=np.uint32) % np.uint32(d)
    msgs = [table[j] for j in idx]
    if kind == "g2pubs":
        pks, _ = eng.g2_mul_generator_batch(sks, n)
        sigs, _ = eng.g2pubs_sign_batch(msgs, sks)
    else:
        pks, _ = eng.g1_mul_generator_batch(sks, n)
        sigs, _ = eng.g1pubs_sign_batch(msgs, sks)
    return table, idx, eng.PackedMsgs(msgs), np.asarray(pks, np.uint8).tobytes(), np.asarray(sigs, np.uint8).tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("a", "bc", "abc"), default="abc")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", default="1024,4096,16384,65536")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_rlc_grouped.log"))
    args = ap.parse_args()
    from bls_amd import engine as eng
    eng.init(0)
    eng.set_option("rlc_min", 0)
    parent = {}
    if args.parent:
        for l in open(args.parent):
            t = l.split()
            if len(t) >= 6 and t[0] in ("g2pubs", "g1pubs", "bad:g2pubs", "bad:g1pubs"):
                parent[(t[0], int(t[1]), int(t[2]))] = (float(t[4]), float(t[5]))
    lines = ["# %s  BLSMI_LIB=%s  reps=%d (median; the legs of one build interleaved), host buffers" % (eng.version(), os.environ.get("BLSMI_LIB", "-"), args.reps),
             "# a = *_verify_batch_rlc_grouped, b = *_verify_batch_rlc at rlc_min = 0, c = *_verify_batch (b, c: messages expanded); pb, pc = b, c of the parent commit's build (%s)" % (args.parent or "-"),
             "# kind n d  a_ms  b_ms  c_ms  pb_ms  pc_ms  pb/a  pc/a"]

    def emit(l):
        print(l, flush=True)
        lines.append(l)

    def measure(kind, table, idx, packed, pks, sigs, want_comb):
        g = eng.g2pubs_verify_batch_rlc_grouped if kind == "g2pubs" else eng.g1pubs_verify_batch_rlc_grouped
        r = eng.g2pubs_verify_batch_rlc if kind == "g2pubs" else eng.g1pubs_verify_batch_rlc
        v = eng.g2pubs_verify_batch if kind == "g2pubs" else eng.g1pubs_verify_batch
        calls = {}
        if "a" in args.only:
            calls["a"] = lambda: g(table, idx, pks, sigs)[2]
        if "b" in args.only:
            calls["b"] = lambda: r(packed, pks, sigs)[2]
            calls["c"] = lambda: int(bool(np.all(v(packed, pks, sigs)[0])))
        for fn in calls.values():                                              # warm-up; the (combined) verdict is what the shape says
            assert fn() == want_comb
        ms = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, fn in calls.items():
                t = time.perf_counter(); fn(); ms[k].append((time.perf_counter() - t) * 1e3)
        return {k: statistics.median(x) for k, x in ms.items()}

    rows = {}

    def row(tag, n, d, m):
        a, b, c = m.get("a"), m.get("b"), m.get("c")
        pb, pc = parent.get((tag, n, d), (None, None))
        rows[(tag, n, d)] = (a, b, c, pb, pc)
        f = lambda x: "%9.3f" % x if x is not None else "        -"
        q = lambda x: "%6.2f" % (x / a) if a and x else "     -"
        return "%s %6d %6d %s %s %s %s %s %s %s" % (tag, n, d, f(a), f(b), f(c), f(pb), f(pc), q(pb), q(pc))

    sizes = [int(x) for x in args.sizes.split(",")]
    for kind in ("g2pubs", "g1pubs"):
        for n in sizes:
            for d in sorted({1, min(64, n), n // 8, n}):
                table, idx, packed, pks, sigs = batch(eng, kind, n, d)
                emit(row(kind, n, d, measure(kind, table, idx, packed, pks, sigs, 1)))
    # one bad tuple: the combined check fails, then the per-tuple path
    N, D = max(sizes), 64
    for kind in ("g2pubs", "g1pubs"):
        table, idx, packed, pks, sigs = batch(eng, kind, N, D)
        bad = bytearray(sigs); w = len(sigs) // N
        bad[w * 5:w * 6] = sigs[w * 6:w * 7]
        emit(row("bad:" + kind, N, D, measure(kind, table, idx, packed, pks, bytes(bad), 0)))
    if "a" in args.only and parent:
        emit("#")
        for kind in ("g2pubs", "g1pubs"):
            a, _, _, pb, pc = rows[(kind, N, D)]
            emit("# %s %d x %d: grouped %.2f ms, parent _rlc %.2f ms (%.2fx), parent verify_batch %.2f ms (%.2fx): the grouped form is %s than the parent's _rlc"
                 % (kind, N, D, a, pb, pb / a, pc, pc / a, "FASTER" if a < pb else "NOT faster"))
            lose = [(n, d) for n in sizes for d in sorted({1, min(64, n), n // 8, n}) if rows[(kind, n, d)][3] is not None and rows[(kind, n, d)][0] >= rows[(kind, n, d)][3]]
            emit("# %s: shapes where the grouped form does not beat the parent's _rlc (d approaching n): %s" % (kind, ", ".join("%d x %d" % x for x in lose) or "none"))
            ba = rows[("bad:" + kind, N, D)]
            emit("# %s one bad tuple at %d x %d: grouped %.2f ms against %.2f ms all valid (+%.2f ms); parent _rlc with the bad tuple %.2f ms, parent verify_batch %.2f ms"
                 % (kind, N, D, ba[0], a, ba[0] - a, ba[3], ba[4]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
