#!/usr/bin/env python3
"""The block-locating randomised batch verification against the plain forms -> profiles/r09_rlc_locate.log.

One MI355X, one process, host buffers, median of 10 calls, the legs of a shape interleaved:
  l  blsmi_g?pubs_verify_batch_rlc_locate, block = 0 (automatic)
  r  blsmi_g?pubs_verify_batch_rlc on the same tuples, "rlc_min" = 0
  v  blsmi_g?pubs_verify_batch on the same
Shapes: g2pubs and g1pubs at 16 384 and 65 536 tuples; all valid, one bad tuple, 16 bad tuples in 16 different blocks.  Then the sweep of
`block` (64 .. 4 096) at the largest size with one bad tuple, which is what the automatic rule (locate_plan.h) is set by.
r and v are compared on a build of the PARENT commit, in two runs on the same machine, one after the other:
  BLSMI_LIB=<parent build> tools/rlc_locate_bench.py --only rv --out parent.log        (that library has no leg l)
  tools/rlc_locate_bench.py --parent parent.log                                         (l, r, v on this build + the parent's r, v per shape)
Each median comes with the spread (max - min of the 10) of its leg; the second run states whether the all-valid l equals the parent's r
within those spreads, and the ratios with bad tuples.  --trace-one runs a single failing call of the largest g2pubs shape and nothing
else (for a kernel trace of its own).

usage: tools/rlc_locate_bench.py [--only l|rv|lrv] [--parent FILE] [--reps 10] [--sizes 16384,65536] [--no-sweep] [--trace-one] [--out FILE]
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
SWEEP = (64, 128, 256, 512, 1024, 2048, 4096)


def batch(eng, kind, n):
    sks = b"".join(hashlib.sha256(b"bench-sk-%d" % i).digest()[:31].rjust(32, b"\0") for i in range(n))
    msgs = [b"bench message %d" % j for j in range(n)]
    if kind == "g2pubs":
        pks, _ = eng.g2_mul_generator_batch(sks, n)
        sigs, _ = eng.g2pubs_sign_batch(msgs, sks)
    else:
        pks, _ = eng.g1_mul_generator_batch(sks, n)
        sigs, _ = eng.g1pubs_sign_batch(msgs, sks)
    return eng.PackedMsgs(msgs), np.asarray(pks, np.uint8).tobytes(), np.asarray(sigs, np.uint8).tobytes()


def corrupt(sigs, n, positions):
    """the signatures with those of `positions` replaced by their neighbours'"""
    b = bytearray(sigs); w = len(sigs) // n
    for i in positions:
        j = i + 1 if i + 1 < n else i - 1
        b[w * i:w * (i + 1)] = sigs[w * j:w * (j + 1)]
    return bytes(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("l", "rv", "lrv"), default="lrv")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", default="16384,65536")
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--trace-one", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_rlc_locate.log"))
    args = ap.parse_args()
    from bls_amd import engine as eng
    eng.init(0)
    eng.set_option("rlc_min", 0)
    sizes = [int(x) for x in args.sizes.split(",")]
    if args.trace_one:
        n = max(sizes)
        packed, pks, sigs = batch(eng, "g2pubs", n)
        bad = corrupt(sigs, n, [n // 2 + 3])
        ok, _, comb, re_ = eng.g2pubs_verify_batch_rlc_locate(packed, pks, bad)
        print("trace-one g2pubs n=%d combined=%d rechecked=%d zeros=%d" % (n, comb, re_, int(n - ok.sum())))
        return
    parent = {}
    if args.parent:
        for l in open(args.parent):
            t = l.split()
            if len(t) >= 8 and not t[0].startswith("#"):
                parent[(t[0], t[1], int(t[2]))] = (float(t[5]), float(t[6]), float(t[7]), float(t[8]))
    lines = ["# %s  BLSMI_LIB=%s  reps=%d (median and spread = max - min; the legs of one build interleaved), host buffers" % (eng.version(), os.environ.get("BLSMI_LIB", "-"), args.reps),
             "# l = *_verify_batch_rlc_locate (block = 0), r = *_verify_batch_rlc at rlc_min = 0, v = *_verify_batch; pr, pv = r, v of the parent commit's build (%s)" % (args.parent or "-"),
             "# kind shape n  l_ms l_spread  r_ms r_spread  v_ms v_spread  pr_ms pr_spread  pv_ms pv_spread  pr/l  pv/l"]

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

    def legs(kind, packed, pks, sigs, n, nbad, block=0):
        loc = getattr(eng, kind + "_verify_batch_rlc_locate", None)
        r = getattr(eng, kind + "_verify_batch_rlc")
        v = getattr(eng, kind + "_verify_batch")

        def run_l():
            ok, _, comb, re_ = loc(packed, pks, sigs, None, None, block)
            assert comb == (0 if nbad else 1) and int(n - ok.sum()) == nbad, (comb, re_)
            return re_

        def run_r():
            ok, _, comb = r(packed, pks, sigs)
            assert comb == (0 if nbad else 1) and int(n - ok.sum()) == nbad

        def run_v():
            assert int(n - v(packed, pks, sigs)[0].sum()) == nbad
        calls = {}
        if "l" in args.only:
            calls["l"] = run_l
        if "r" in args.only:
            calls["r"] = run_r
            calls["v"] = run_v
        return calls

    rows = {}

    def row(kind, shape, n, m):
        z = (None, None)
        l, r, v = m.get("l", z), m.get("r", z), m.get("v", z)
        p = parent.get((kind, shape, n))
        pr, pv = ((p[0], p[1]), (p[2], p[3])) if p else (z, z)
        rows[(kind, shape, n)] = (l, r, v, pr, pv)
        f = lambda x: "%8.3f %6.3f" % x if x[0] is not None else "       -      -"   # noqa: E731
        q = lambda x: "%6.2f" % (x[0] / l[0]) if l[0] and x[0] else "     -"           # noqa: E731
        return "%s %s %6d  %s  %s  %s  %s  %s  %s %s" % (kind, shape, n, f(l), f(r), f(v), f(pr), f(pv), q(pr), q(pv))

    data = {}
    for kind in ("g2pubs", "g1pubs"):
        for n in sizes:
            packed, pks, sigs = batch(eng, kind, n)
            data[(kind, n)] = (packed, pks, sigs)
            step = max(2 * max(64, -(-n // 256)), n // 16)                        # 16 positions in 16 different automatic blocks
            for shape, positions in (("valid", []), ("bad1", [n // 2 + 3]), ("bad16", [5 + step * j for j in range(16) if 5 + step * j < n])):
                s = corrupt(sigs, n, positions) if positions else sigs
                emit(row(kind, shape, n, measure(legs(kind, packed, pks, s, n, len(positions)))))
    N = max(sizes)
    if "l" in args.only and not args.no_sweep:
        emit("# block sweep, one bad tuple at %d tuples (l alone; rechecked = block)" % N)
        for kind in ("g2pubs", "g1pubs"):
            packed, pks, sigs = data[(kind, N)]
            s = corrupt(sigs, N, [N // 2 + 3])
            loc = getattr(eng, kind + "_verify_batch_rlc_locate")
            calls = {}
            for b in SWEEP:
                calls[b] = (lambda b=b: loc(packed, pks, s, None, None, b))
            m = measure(calls)
            for b in SWEEP:
                emit("sweep %s %6d block %5d  %8.3f %6.3f" % (kind, N, b, m[b][0], m[b][1]))
            best = min(SWEEP, key=lambda b: m[b][0])
            emit("# %s: fastest block %d (%.3f ms); the automatic rule gives %d (%.3f ms)" % (kind, best, m[best][0], max(64, -(-N // 256)), m.get(max(64, -(-N // 256)), (float("nan"),))[0]))
    if "l" in args.only and parent:
        emit("#")
        for kind in ("g2pubs", "g1pubs"):
            for n in sizes:
                l, _, _, pr, pv = rows[(kind, "valid", n)]
                d = l[0] - pr[0]
                emit("# %s %d all valid: locate %.3f ms (spread %.3f), parent _rlc %.3f ms (spread %.3f): difference %+.3f ms, %s the spreads of the two legs"
                     % (kind, n, l[0], l[1], pr[0], pr[1], d, "WITHIN" if abs(d) <= max(l[1], pr[1]) else "BEYOND"))
                for shape in ("bad1", "bad16"):
                    l, _, _, pr, pv = rows[(kind, shape, n)]
                    emit("# %s %d %s: locate %.3f ms, parent _rlc %.3f ms (%.2fx), parent verify_batch %.3f ms (%.2fx): locate is %s than the parent's failing _rlc"
                         % (kind, n, shape, l[0], pr[0], pr[0] / l[0], pv[0], pv[0] / l[0], "FASTER" if l[0] < pr[0] else "NOT faster"))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
