#!/usr/bin/env python3
"""Randomised batch verification against verify_batch on the same host inputs, in one process (include/blsmi.h: *_verify_batch_rlc).
For both packages and each size: the two calls alternated, median of --reps warm calls each, verifies/s and the ratio; then the failure
path (one bad tuple) at 4 096 and 65 536.  "rlc_min" is set to 0 so that every size takes the combined check.
usage: python tools/rlc_bench.py [--reps 10] [--sizes 1024,2048,4096,16384,32768,65536]"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def batch(eng, kind, n):
    sks = b"".join(hashlib.sha256(b"rlc-bench-%d" % i).digest()[:31].rjust(32, b"\0") for i in range(n))
    msgs = [hashlib.sha256(b"m%d" % i).digest() for i in range(n)]
    if kind == "g2pubs":
        pks, _ = eng.g2_mul_generator_batch(sks, n); sigs, _ = eng.g2pubs_sign_batch(msgs, sks)
    else:
        pks, _ = eng.g1_mul_generator_batch(sks, n); sigs, _ = eng.g1pubs_sign_batch(msgs, sks)
    return msgs, np.asarray(pks, np.uint8).tobytes(), np.asarray(sigs, np.uint8).tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", default="1024,2048,4096,16384,32768,65536")
    ap.add_argument("--fail-sizes", default="4096,65536")
    a = ap.parse_args()
    from bls_amd import engine as eng
    eng.init(0)
    eng.set_option("rlc_min", 0)
    print(eng.version())
    res = {"rows": [], "fail": []}
    for kind in ("g2pubs", "g1pubs"):
        vb = eng.g2pubs_verify_batch if kind == "g2pubs" else eng.g1pubs_verify_batch
        rl = eng.g2pubs_verify_batch_rlc if kind == "g2pubs" else eng.g1pubs_verify_batch_rlc
        for n in [int(x) for x in a.sizes.split(",")]:
            msgs, pks, sigs = batch(eng, kind, n)
            for _ in range(2):
                vb(msgs, pks, sigs); rl(msgs, pks, sigs)
            tv, tr, combs = [], [], set()
            for _ in range(a.reps):
                t0 = time.perf_counter(); ok, _ = vb(msgs, pks, sigs); tv.append(time.perf_counter() - t0)
                assert ok.all()
                t0 = time.perf_counter(); ok, _, c = rl(msgs, pks, sigs); tr.append(time.perf_counter() - t0)
                assert ok.all(); combs.add(c)
            mv, mr = statistics.median(tv), statistics.median(tr)
            row = {"kind": kind, "n": n, "verify_batch_ms": round(mv * 1e3, 3), "rlc_ms": round(mr * 1e3, 3), "verify_batch_per_s": round(n / mv),
                   "rlc_per_s": round(n / mr), "speedup": round(mv / mr, 3), "combined": sorted(combs),
                   "spread_ms": [round((max(tv) - min(tv)) * 1e3, 3), round((max(tr) - min(tr)) * 1e3, 3)]}
            res["rows"].append(row)
            print("%-7s n=%6d  verify_batch %8.3f ms (%9.0f /s)  rlc %8.3f ms (%9.0f /s)  x%.2f  combined=%s" % (kind, n, mv * 1e3, n / mv, mr * 1e3, n / mr, mv / mr, sorted(combs)), flush=True)
            if n in [int(x) for x in a.fail_sizes.split(",")]:
                m = list(msgs); m[n // 3] = b"forged"
                rl(m, pks, sigs)
                tf = []
                for _ in range(max(3, a.reps // 2)):
                    t0 = time.perf_counter(); ok, _, c = rl(m, pks, sigs); tf.append(time.perf_counter() - t0)
                    assert c == 0 and not ok[n // 3] and ok.sum() == n - 1
                mf = statistics.median(tf)
                res["fail"].append({"kind": kind, "n": n, "rlc_fail_ms": round(mf * 1e3, 3), "verify_batch_ms": round(mv * 1e3, 3), "ratio_to_verify_batch": round(mf / mv, 3)})
                print("%-7s n=%6d  one bad tuple: rlc %8.3f ms = %.2f x verify_batch" % (kind, n, mf * 1e3, mf / mv), flush=True)
    print("RLC_BENCH " + json.dumps(res))


if __name__ == "__main__":
    main()
