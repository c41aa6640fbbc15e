#!/usr/bin/env python3
"""Kernel times of the batch point validation (blsmi 0.14) beside the decompression kernels', from the library's own profile
(blsmi_set_profiling / blsmi_last_profile: HIP events around each kernel on the launch stream).

Per n (default 4 096 and 65 536), on n subgroup points (sk_i * generator, computed on the device):
    k_g?_check       blsmi_g?_check_batch      check = 1, affine records
    k_g?_check_jac   blsmi_g?_check_batch_jac  check = 1, in-memory records (z = 1: the arithmetic does not look at the value of z)
    k_g?_decompress  blsmi_g?_decompress_batch check = 1 on the compressed forms of the same points, latency threshold 0 so that the
                     subgroup test runs inside the kernel and not as a level program -- the yardstick: the same test plus a square root
Each is run --reps times (default 3) after one warm-up, the kinds interleaved; one JSON line per (n, kernel) with the times, their median and
spread (max - min).  G2 takes the lane-pair kernels by default; run again with BLSMI_LAYOUT=single in the environment for the one-lane ones.
BLSMI_LIB=<another build> times that build's kernels (a build without the check entry points gives the decompression rows only).

    python tools/point_check_bench.py [--sizes 4096,65536] [--reps 3] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bls_amd import engine  # noqa: E402


def profile(lib, buf):
    lib.blsmi_last_profile(buf, ctypes.c_size_t(len(buf)))
    out = {}
    for item in buf.value.decode().split(";"):
        if "=" in item:
            k, v = item.rsplit("=", 1)
            out[k.strip()] = out.get(k.strip(), 0.0) + float(v)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,65536")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    engine.init(0)
    lib = engine._lib()
    have_check = hasattr(lib, "blsmi_g1_check_batch")
    buf = ctypes.create_string_buffer(1 << 16)
    rng = np.random.default_rng(20260)
    lines = []
    for n in [int(s) for s in a.sizes.split(",")]:
        sk = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        sk[:, 0] &= 0x3f                                                      # below r
        sk = sk.tobytes()
        work = []
        for g, pb in (("g1", 96), ("g2", 192)):
            pts, inf = getattr(engine, g + "_mul_generator_batch")(sk, n)
            assert not inf.any()
            pts = pts.tobytes()
            jac = getattr(engine, g + "_mul_generator_batch_jac")(sk, n).tobytes()
            comp = getattr(engine, g + "_compress_batch")(pts, n).tobytes()
            if have_check:
                work.append(("k_%s_check" % g, lambda g=g, pts=pts: getattr(engine, g + "_check_batch")(pts, n, None, 1)))
                work.append(("k_%s_check_jac" % g, lambda g=g, jac=jac: getattr(engine, g + "_check_batch_jac")(jac, n, 1)))
            work.append(("k_%s_decompress" % g, lambda g=g, comp=comp: getattr(engine, g + "_decompress_batch")(comp, n, 1)[2]))
        engine.set_latency_threshold(0)
        times = {}
        try:
            for rep in range(a.reps + 1):                                     # (rep 0: warm-up)
                lib.blsmi_set_profiling(1 if rep else 0)
                for name, call in work:
                    st = call()
                    assert not np.asarray(st).any(), name                     # subgroup points: status / err 0 throughout
                    if rep:
                        prof = profile(lib, buf)
                        hit = [k for k in prof if k == name or k == name + "_pair"]
                        assert len(hit) == 1, (name, prof)
                        times.setdefault(hit[0], []).append(prof[hit[0]])
        finally:
            lib.blsmi_set_profiling(0)
            engine.set_latency_threshold(8192)
        for k, v in times.items():
            lines.append(json.dumps({"n": n, "kernel": k, "layout": os.environ.get("BLSMI_LAYOUT", "default"), "ms": [round(x, 4) for x in v],
                                     "median_ms": round(float(np.median(v)), 4), "spread_ms": round(max(v) - min(v), 4)}))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
