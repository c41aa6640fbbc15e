#!/usr/bin/env python3
"""Randomised pairing-product batches (include/blsmi.h: blsmi_pairing_product_batch_rlc*) against the per-item call of 0.10, points resident
on the device.  For each shape the two calls alternate in one process; after warm-up of both, the median of --reps calls and the spread
(max - min) of
  rlc   blsmi_pairing_product_batch_rlc_dev over (P, table, q_idx), with the per-stage split of one profiled call (blsmi_last_profile);
  item  blsmi_pairing_product_batch_dev over the same pairs, the table expanded per pair, verdicts only
with every item holding ("valid") and with one item that does not ("onebad": the rlc call then runs the per-item path as well).
Shapes, m items x k pairs: groth = three shared table entries and one private per item (k = 4), kzg = both entries shared (k = 2),
none = the groth pairs with q_idx = NULL (every pair its own entry: nothing shared).
The singleton by-pass's criterion: at the first groth shape, the rlc call against
blsmi_debug_pairing_product_batch_rlc_dev_nosplit (every group through the weighted segmented sum), alternating, same statistics.
usage: python tools/pprod_rlc_bench.py [--reps 20] [--shapes groth:16384,groth:65536,kzg:16384,none:16384,groth:2048] [--out FILE]"""
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

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
X, Y, Z = 0x1234567 + 3 * 2 ** 70, 0x7654321 + 5 * 2 ** 90, 0xabcdef + 7 * 2 ** 60


def read_profile(lib):
    buf = ctypes.create_string_buffer(1 << 16)
    lib.blsmi_last_profile(buf, ctypes.c_size_t(len(buf)))
    out = {}
    for item in buf.value.decode().split(";"):
        if "=" in item:
            k, v = item.split("=")
            out[k] = round(out.get(k, 0.0) + float(v), 4)
    return out


def alternate(fa, fb, reps):
    ta, tb = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); fa(); ta.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter(); fb(); tb.append((time.perf_counter() - t0) * 1e3)
    return [(round(statistics.median(t), 3), round(max(t) - min(t), 3)) for t in (ta, tb)]


def be32(vals):
    return b"".join((v % R).to_bytes(32, "big") for v in vals)


def make(eng, kind, m, bad):
    """-> (g1 bytes, table bytes, q_idx or None, k): items that hold, item 0 spoiled when `bad`"""
    rng = np.random.default_rng(m + len(kind))
    rnd = lambda: int.from_bytes(rng.bytes(31), "big")
    xinv = pow(X, -1, R)
    s1, s2 = [], [X, Y, Z] if kind != "kzg" else [X, Y]
    q = []
    for j in range(m):
        off = 1 if bad and j == 0 else 0
        if kind == "kzg":
            s = rnd()
            s1 += [s * Y + off, -(s * X)]
            q += [0, 1]
        else:
            a, b, t, u = rnd(), rnd(), rnd(), rnd()
            s1 += [a + off, -((a * b + t * Y + u * Z) * xinv), t, u]
            s2.append(b)
            q += [3 + j, 0, 1, 2]
    g1, _ = eng.g1_mul_generator_batch(be32(s1), len(s1))
    tab, _ = eng.g2_mul_generator_batch(be32(s2), len(s2))
    g1, tab = np.frombuffer(bytes(g1), dtype=np.uint8).reshape(-1, 96), np.frombuffer(bytes(tab), dtype=np.uint8).reshape(-1, 192)
    q = np.array(q, dtype=np.uint32)
    if kind == "none":
        return g1, tab[q], None, 4
    return g1, tab, q, 2 if kind == "kzg" else 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="groth:16384,groth:65536,kzg:16384,none:16384,groth:2048")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from bls_amd import _native, engine as eng
    eng.init(0)
    lib = _native.load()
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("%s  reps %d (median, spread = max - min, ms; the two calls alternate)" % (eng.version(), a.reps))
    rows, criterion = [], None
    for shape in a.shapes.split(","):
        kind, m = shape.split(":")
        m = int(m)
        for mode in ("valid", "onebad"):
            g1, tab, q, k = make(eng, kind, m, mode == "onebad")
            n, nq = g1.shape[0], tab.shape[0]
            expanded = tab if q is None else tab[q]
            off = eng.seg_offsets([k] * m)
            t = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)
            d1, dt, dx, d_off = t(g1), t(tab), t(expanded), t(off)
            dq = t(q) if q is not None else None
            d_rlc = torch.zeros(m, dtype=torch.uint8, device=dev)
            d_item = torch.zeros(m, dtype=torch.uint8, device=dev)
            comb = []
            f_rlc = lambda nosplit=False: comb.append(eng.pairing_product_batch_rlc_dev(d1.data_ptr(), dt.data_ptr(), nq, dq.data_ptr() if dq is not None else 0, n, d_off.data_ptr(), m,
                                                                                         d_rlc.data_ptr(), nosplit=nosplit))
            f_item = lambda: eng.pairing_product_batch_dev(d1.data_ptr(), dx.data_ptr(), n, d_off.data_ptr(), m, 0, d_item.data_ptr())
            for _ in range(2):
                f_rlc(); f_item()
            want = [0 if (mode == "onebad" and j == 0) else 1 for j in range(m)]
            agree = d_rlc.cpu().numpy().tolist() == d_item.cpu().numpy().tolist() == want and set(comb) == {1 if mode == "valid" else 0}
            (rlc, rlc_sp), (item, item_sp) = alternate(f_rlc, f_item, a.reps)
            read_profile(lib); lib.blsmi_set_profiling(1); f_rlc(); lib.blsmi_set_profiling(0)
            prof = read_profile(lib)
            row = {"shape": "%s %dx%d" % (kind, m, k), "mode": mode, "pairs": n, "table": nq, "rlc_ms": rlc, "rlc_spread_ms": rlc_sp, "item_ms": item, "item_spread_ms": item_sp,
                   "item_over_rlc": round(item / rlc, 2), "win_beyond_spread": bool(item - rlc > max(rlc_sp, item_sp)), "verdicts_agree": bool(agree), "rlc_profile_ms": prof}
            rows.append(row)
            say(json.dumps(row))
            if criterion is None and kind == "groth" and mode == "valid":
                for _ in range(2):
                    f_rlc(True)
                (sp, sp_s), (ns, ns_s) = alternate(f_rlc, lambda: f_rlc(True), a.reps)
                read_profile(lib); lib.blsmi_set_profiling(1); f_rlc(True); lib.blsmi_set_profiling(0)
                criterion = {"shape": row["shape"], "singleton_groups": m, "split_ms": sp, "split_spread_ms": sp_s, "nosplit_ms": ns, "nosplit_spread_ms": ns_s,
                             "bypass_stays": bool(ns - sp > max(sp_s, ns_s)), "nosplit_profile_ms": read_profile(lib)}
                say("SINGLETON_CRITERION " + json.dumps(criterion))
    say("PPROD_RLC_BENCH " + json.dumps({"version": eng.version(), "reps": a.reps, "rows": rows, "singleton_criterion": criterion}))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
