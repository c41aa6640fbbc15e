#!/usr/bin/env python3
"""The grouped randomised batch verification that finds the bad tuples by cells against the grouped and the plain forms
-> profiles/r10_rlc_grouped_locate.log.

One MI355X, one process, host buffers, median of 10 calls, the legs of a shape interleaved:
  c  blsmi_g?pubs_verify_batch_rlc_grouped_locate over a table of d messages, block = 0 (automatic)
  g  blsmi_g?pubs_verify_batch_rlc_grouped on the same tuples
  v  blsmi_g?pubs_verify_batch on the same, the messages expanded
Shapes, g2pubs and g1pubs: 65 536 x 64 all valid, with one bad tuple, with 16 bad tuples in 16 different cells; 65 536 x 8 192 all valid;
16 384 x 64 all valid and with one bad tuple.
g and v are compared on a build of the PARENT commit, in two runs on the same machine, one after the other:
  BLSMI_LIB=<parent build> tools/rlc_grouped_locate_bench.py --only gv --out parent.log     (that library has no leg c)
  tools/rlc_grouped_locate_bench.py --parent parent.log                                      (c, g, v on this build + the parent's g, v per shape)
Each median comes with the spread (max - min of the 10) of its leg.  The second run states, per package, whether the call with one bad
tuple at the largest shape is below the parent's failing grouped call by more than the sum of the two legs' spreads, and the difference
of the call that holds to the parent's.  --trace-one fail|hold|grouped-hold runs a single call of the largest g2pubs shape x 64 and nothing
else (for a kernel trace of its own): the new form with one bad tuple, the new form all valid, the grouped form all valid.

usage: tools/rlc_grouped_locate_bench.py [--only c|gv|cgv] [--parent FILE] [--reps 10] [--shapes 65536x64,65536x8192,16384x64] [--trace-one WHICH] [--out FILE]
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


def corrupt(sigs, n, positions):
    """the signatures with those of `positions` replaced by their neighbours' (another message's, with d > 1)"""
    b = bytearray(sigs); w = len(sigs) // n
    for i in positions:
        j = i + 1 if i + 1 < n else i - 1
        b[w * i:w * (i + 1)] = sigs[w * j:w * (j + 1)]
    return bytes(b)


def shapes_of(n, d):
    """valid / bad1 / bad16 at d = 64, valid alone elsewhere; tuple i belongs to message i % d, so 16 neighbours sit in 16 groups: 16 cells"""
    if d != 64:
        return (("valid", []),)
    out = (("valid", []), ("bad1", [n // 2 + 3]))
    return out + ((("bad16", [n // 4 + j for j in range(16)]),) if n >= 65536 else ())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("c", "gv", "cgv"), default="cgv")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="65536x64,65536x8192,16384x64")
    ap.add_argument("--trace-one", choices=("fail", "hold", "grouped-hold"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_rlc_grouped_locate.log"))
    args = ap.parse_args()
    from bls_amd import engine as eng
    eng.init(0)
    shapes = [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")]
    if args.trace_one:
        n = max(s[0] for s in shapes)
        table, idx, _, pks, sigs = batch(eng, "g2pubs", n, 64)
        if args.trace_one == "grouped-hold":
            ok, _, comb = eng.g2pubs_verify_batch_rlc_grouped(table, idx, pks, sigs)
            print("trace-one grouped-hold g2pubs n=%d d=64 combined=%d zeros=%d" % (n, comb, int(n - ok.sum())))
            return
        s = corrupt(sigs, n, [n // 2 + 3]) if args.trace_one == "fail" else sigs
        ok, _, comb, re_ = eng.g2pubs_verify_batch_rlc_grouped_locate(table, idx, pks, s)
        print("trace-one %s g2pubs n=%d d=64 combined=%d rechecked=%d zeros=%d" % (args.trace_one, n, comb, re_, int(n - ok.sum())))
        return
    parent = {}
    if args.parent:
        for l in open(args.parent):
            t = l.split()
            if len(t) >= 10 and not t[0].startswith("#"):
                parent[(t[0], t[1], int(t[2]), int(t[3]))] = (float(t[6]), float(t[7]), float(t[8]), float(t[9]))
    lines = ["# %s  BLSMI_LIB=%s  reps=%d (median and spread = max - min; the legs of one build interleaved), host buffers" % (eng.version(), os.environ.get("BLSMI_LIB", "-"), args.reps),
             "# c = *_verify_batch_rlc_grouped_locate (block = 0), g = *_verify_batch_rlc_grouped, v = *_verify_batch (messages expanded); pg, pv = g, v of the parent commit's build (%s)" % (args.parent or "-"),
             "# kind shape n d  c_ms c_spread  g_ms g_spread  v_ms v_spread  pg_ms pg_spread  pv_ms pv_spread  pg/c  pv/c  rechecked"]

    def emit(l):
        print(l, flush=True)
        lines.append(l)

    def measure(calls):
        for fn in calls.values():
            fn()                                                                  # warm-up (each call checks its own verdicts)
        ms = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, fn in calls.items():
                t = time.perf_counter(); fn(); ms[k].append((time.perf_counter() - t) * 1e3)
        return {k: (statistics.median(x), max(x) - min(x)) for k, x in ms.items()}

    rechecked = {}

    def legs(kind, shape, table, idx, packed, pks, sigs, n, nbad):
        cl = getattr(eng, kind + "_verify_batch_rlc_grouped_locate", None)
        g = getattr(eng, kind + "_verify_batch_rlc_grouped")
        v = getattr(eng, kind + "_verify_batch")

        def run_c():
            ok, _, comb, re_ = cl(table, idx, pks, sigs)
            assert comb == (0 if nbad else 1) and int(n - ok.sum()) == nbad, (comb, re_)
            rechecked[(kind, shape, n, len(table))] = re_

        def run_g():
            ok, _, comb = g(table, idx, pks, sigs)
            assert comb == (0 if nbad else 1) and int(n - ok.sum()) == nbad

        def run_v():
            assert int(n - v(packed, pks, sigs)[0].sum()) == nbad
        calls = {}
        if "c" in args.only:
            calls["c"] = run_c
        if "g" in args.only:
            calls["g"] = run_g
            calls["v"] = run_v
        return calls

    rows = {}

    def row(kind, shape, n, d, m):
        z = (None, None)
        c, g, v = m.get("c", z), m.get("g", z), m.get("v", z)
        p = parent.get((kind, shape, n, d))
        pg, pv = ((p[0], p[1]), (p[2], p[3])) if p else (z, z)
        rows[(kind, shape, n, d)] = (c, g, v, pg, pv)
        f = lambda x: "%8.3f %6.3f" % x if x[0] is not None else "       -      -"   # noqa: E731
        q = lambda x: "%6.2f" % (x[0] / c[0]) if c[0] and x[0] else "     -"           # noqa: E731
        re_ = rechecked.get((kind, shape, n, d))
        return "%s %s %6d %5d  %s  %s  %s  %s  %s  %s %s  %s" % (kind, shape, n, d, f(c), f(g), f(v), f(pg), f(pv), q(pg), q(pv), re_ if re_ is not None else "-")

    for kind in ("g2pubs", "g1pubs"):
        for n, d in shapes:
            table, idx, packed, pks, sigs = batch(eng, kind, n, d)
            for shape, positions in shapes_of(n, d):
                s = corrupt(sigs, n, positions) if positions else sigs
                emit(row(kind, shape, n, d, measure(legs(kind, shape, table, idx, packed, pks, s, n, len(positions)))))
    if "c" in args.only and parent:
        emit("#")
        N = max(s[0] for s in shapes)
        for kind in ("g2pubs", "g1pubs"):
            for (k, shape, n, d), (c, _, _, pg, pv) in rows.items():
                if k != kind or pg[0] is None:
                    continue
                if shape == "valid":
                    emit("# %s %d x %d all valid: cells %.3f ms (spread %.3f), parent grouped %.3f ms (spread %.3f): difference %+.3f ms"
                         % (kind, n, d, c[0], c[1], pg[0], pg[1], c[0] - pg[0]))
                else:
                    emit("# %s %d x %d %s: cells %.3f ms, parent grouped %.3f ms (%.2fx), parent verify_batch %.3f ms (%.2fx)"
                         % (kind, n, d, shape, c[0], pg[0], pg[0] / c[0], pv[0], pv[0] / c[0]))
            key = (kind, "bad1", N, 64)
            if key in rows and rows[key][3][0] is not None:
                c, _, _, pg, _ = rows[key]
                gain, need = pg[0] - c[0], c[1] + pg[1]
                emit("# %s one bad tuple at %d x 64: cells %.3f ms (spread %.3f) against the parent's failing grouped call %.3f ms (spread %.3f): below it by %.3f ms, the two spreads sum to %.3f ms: condition %s"
                     % (kind, N, c[0], c[1], pg[0], pg[1], gain, need, "MET" if gain > need else "NOT met"))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
