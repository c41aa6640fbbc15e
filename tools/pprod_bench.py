#!/usr/bin/env python3
"""Pairing products (include/blsmi.h: blsmi_pairing_product_batch*) timed for m segments of k pairs each, points resident on the device.
For each shape, after warm-up, the median of --reps calls and the spread (max - min) of
  a  blsmi_pairing_product_batch_dev, with the per-kernel split of one profiled call (blsmi_last_profile);
  b  blsmi_pairing_batch_dev of the same m k pairs -- the same Miller work, k times the final exponentiations, no product stage;
  c  what a caller could do before 0.10: blsmi_miller_loop_batch, m calls of blsmi_fq12_product, blsmi_final_exponentiation_batch (host
     forms: they have no device form; --c-reps calls).
--legs picks the legs; a library without the product entry points (BLSMI_LIB=<an older build>) runs leg b only.  --parent-b FILE reads the
PPROD_BENCH line of such a run and adds, per shape, a / parent b and whether a stays within parent b + parent b's spread.
usage: python tools/pprod_bench.py [--reps 20] [--shapes 2048x4,4096x2,16384x4,1x8192] [--legs a,b,c] [--parent-b FILE]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def read_profile(lib):
    buf = ctypes.create_string_buffer(1 << 16)
    lib.blsmi_last_profile(buf, ctypes.c_size_t(len(buf)))
    out = {}
    for item in buf.value.decode().split(";"):
        if "=" in item:
            k, v = item.split("=")
            out[k] = round(out.get(k, 0.0) + float(v), 4)
    return out


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 3), round(max(ts) - min(ts), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--c-reps", type=int, default=2)
    ap.add_argument("--shapes", default="2048x4,4096x2,16384x4,1x8192")
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--parent-b", default=None)
    a = ap.parse_args()
    import torch
    from bls_amd import _native, engine as eng
    eng.init(0)
    lib = _native.load()
    legs = set(a.legs.split(","))
    if not hasattr(lib, "blsmi_pairing_product_batch_dev"):
        legs &= {"b"}
    print(eng.version(), "legs", sorted(legs), flush=True)
    parent = {}
    if a.parent_b:
        for line in open(a.parent_b):
            if line.startswith("PPROD_BENCH "):
                parent = {r["shape"]: r for r in json.loads(line[len("PPROD_BENCH "):])["rows"]}
    dev = torch.device("cuda", 0)
    rows = []
    for shape in a.shapes.split(","):
        m, k = (int(x) for x in shape.split("x"))
        n = m * k
        rng = np.random.default_rng(n + k)
        sk = rng.integers(0, 256, size=(2, n, 32), dtype=np.uint8); sk[:, :, 0] &= 0x3f
        g1, _ = eng.g1_mul_generator_batch(sk[0].reshape(-1).tobytes(), n)
        g2, _ = eng.g2_mul_generator_batch(sk[1].reshape(-1).tobytes(), n)
        off = eng.seg_offsets([k] * m)
        d1, d2 = torch.from_numpy(g1.reshape(-1).copy()).to(dev), torch.from_numpy(g2.reshape(-1).copy()).to(dev)
        d_off = torch.from_numpy(off.view(np.uint8).copy()).to(dev)
        d_out = torch.zeros(n * 576, dtype=torch.uint8, device=dev)
        d_one = torch.zeros(m, dtype=torch.uint8, device=dev)
        row = {"shape": shape, "m": m, "k": k, "pairs": n}
        if "b" in legs:
            fb = lambda: eng.pairing_batch_dev(d1.data_ptr(), d2.data_ptr(), d_out.data_ptr(), n)
            fb(); fb()
            row["b_ms"], row["b_spread_ms"] = timed(fb, a.reps)
        if "a" in legs:
            fa = lambda: eng.pairing_product_batch_dev(d1.data_ptr(), d2.data_ptr(), n, d_off.data_ptr(), m, d_out.data_ptr(), d_one.data_ptr())
            fa(); fa()
            row["a_ms"], row["a_spread_ms"] = timed(fa, a.reps)
            read_profile(lib); lib.blsmi_set_profiling(1); fa(); lib.blsmi_set_profiling(0)
            row["a_profile_ms"] = read_profile(lib)
            if "b" in legs:
                row["a_over_b"] = round(row["a_ms"] / row["b_ms"], 3)
            pb = parent.get(shape)
            if pb:
                row["parent_b_ms"], row["parent_b_spread_ms"] = pb["b_ms"], pb["b_spread_ms"]
                row["a_over_parent_b"] = round(row["a_ms"] / pb["b_ms"], 3)
                row["a_within_parent_b_plus_spread"] = bool(row["a_ms"] <= pb["b_ms"] + pb["b_spread_ms"])
        if "c" in legs:
            h1, h2 = g1.reshape(-1).tobytes(), g2.reshape(-1).tobytes()

            def fc():
                f = eng.miller_loop_batch(h1, h2, n)
                prods = np.stack([eng.fq12_product(f[j * k:(j + 1) * k]) for j in range(m)])
                return eng.final_exponentiation_batch(prods)
            vc = fc()
            row["c_ms"], row["c_spread_ms"] = timed(fc, a.c_reps)
            if "a" in legs:
                row["c_over_a"] = round(row["c_ms"] / row["a_ms"], 2)
                fa()
                got = d_out.cpu().numpy()[:m * 576].view(np.uint64).reshape(m, 72)
                row["a_equals_c"] = bool(np.array_equal(got, np.asarray(vc).reshape(m, 72)))
        rows.append(row)
        print(json.dumps(row), flush=True)
    print("PPROD_BENCH " + json.dumps({"version": eng.version(), "reps": a.reps, "rows": rows}))


if __name__ == "__main__":
    main()
