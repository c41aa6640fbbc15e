#!/usr/bin/env python3
"""Randomised pairing-product batches that find the bad items by blocks (include/blsmi.h: blsmi_pairing_product_batch_rlc_locate*) against
the form of 0.17 and the per-item call of 0.10, points resident on the device.  For each shape the three calls alternate in one process;
after warm-up of all of them, the median of --reps calls and the spread (max - min), in ms, of
  locate  blsmi_pairing_product_batch_rlc_locate_dev at block = 0, with the per-stage split of one profiled call (blsmi_last_profile);
  rlc     blsmi_pairing_product_batch_rlc_dev over the same arguments;
  item    blsmi_pairing_product_batch_dev over the same pairs, the table expanded per pair, verdicts only
with every item holding ("valid"), with one item that does not ("onebad") and with 16 such items in 16 different blocks ("bad16").
Shapes as tools/pprod_rlc_bench.py: groth = three shared table entries and one private per item (k = 4), kzg = both entries shared
(k = 2), none = the groth pairs with q_idx = NULL.
Criterion 1: at the groth shapes with one bad item, locate is faster than rlc by more than the sum of the two spreads.
The block sweep: at the last groth shape of --sweep-at items with one bad item, block = 0 / 64 / 256 / 1 024 / 4 096 alternate.
usage: python tools/pprod_rlc_locate_bench.py [--reps 20] [--shapes groth:16384,groth:65536,kzg:16384,none:16384,groth:2048] [--sweep-at 65536] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pprod_rlc_bench import R, X, Y, Z, be32, read_profile  # noqa: E402


def alternate(fs, reps):
    ts = [[] for _ in fs]
    for _ in range(reps):
        for f, t in zip(fs, ts):
            t0 = time.perf_counter(); f(); t.append((time.perf_counter() - t0) * 1e3)
    return [(round(statistics.median(t), 3), round(max(t) - min(t), 3)) for t in ts]


def scalars_of(kind, m):
    """-> (G1 scalars, G2 scalars, q_idx, k): items that hold; item j's first G1 scalar is s1[k * j]"""
    rng = np.random.default_rng(m + len(kind))
    rnd = lambda: int.from_bytes(rng.bytes(31), "big")
    xinv = pow(X, -1, R)
    s1, s2 = [], [X, Y, Z] if kind != "kzg" else [X, Y]
    q = []
    for j in range(m):
        if kind == "kzg":
            s = rnd()
            s1 += [s * Y, -(s * X)]
            q += [0, 1]
        else:
            a, b, t, u = rnd(), rnd(), rnd(), rnd()
            s1 += [a, -((a * b + t * Y + u * Z) * xinv), t, u]
            s2.append(b)
            q += [3 + j, 0, 1, 2]
    return s1, s2, np.array(q, dtype=np.uint32), 2 if kind == "kzg" else 4


def auto_block(m):
    return max(64, -(-m // 256))


def bad_items(m, mode):
    if mode == "valid":
        return []
    block = auto_block(m)
    B = -(-m // block)
    if mode == "onebad":
        return [(B // 2) * block + 1]
    return sorted({min(m - 1, ((i * B) // 16) * block + 1) for i in range(16)})   # bad16: one item in each of 16 blocks (fewer where B < 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="groth:16384,groth:65536,kzg:16384,none:16384,groth:2048")
    ap.add_argument("--sweep-at", type=int, default=65536)
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
    say("%s  reps %d (median, spread = max - min, ms; the calls alternate)" % (eng.version(), a.reps))
    rows, sweep = [], None
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)
    for shape in a.shapes.split(","):
        kind, m = shape.split(":")
        m = int(m)
        s1, s2, q, k = scalars_of(kind, m)
        tab, _ = eng.g2_mul_generator_batch(be32(s2), len(s2))
        tab = np.frombuffer(bytes(tab), dtype=np.uint8).reshape(-1, 192)
        expanded = tab[q]
        if kind == "none":
            tab, q = expanded, None
        n, nq = len(s1), tab.shape[0]
        off = eng.seg_offsets([k] * m)
        dt, dx, d_off = t(tab), t(expanded), t(off)
        dq = t(q) if q is not None else None
        for mode in ("valid", "onebad", "bad16"):
            bad = bad_items(m, mode)
            s = list(s1)
            for j in bad:
                s[k * j] += 1
            g1, _ = eng.g1_mul_generator_batch(be32(s), n)
            d1 = t(np.frombuffer(bytes(g1), dtype=np.uint8))
            d_loc, d_rlc, d_item = (torch.zeros(m, dtype=torch.uint8, device=dev) for _ in range(3))
            got = {"loc": [], "rlc": []}
            qp = dq.data_ptr() if dq is not None else 0
            f_loc = lambda block=0: got["loc"].append(eng.pairing_product_batch_rlc_locate_dev(d1.data_ptr(), dt.data_ptr(), nq, qp, n, d_off.data_ptr(), m, d_loc.data_ptr(), block=block))
            f_rlc = lambda: got["rlc"].append(eng.pairing_product_batch_rlc_dev(d1.data_ptr(), dt.data_ptr(), nq, qp, n, d_off.data_ptr(), m, d_rlc.data_ptr()))
            f_item = lambda: eng.pairing_product_batch_dev(d1.data_ptr(), dx.data_ptr(), n, d_off.data_ptr(), m, 0, d_item.data_ptr())
            for _ in range(2):
                f_loc(); f_rlc(); f_item()
            want = np.ones(m, dtype=np.uint8); want[bad] = 0
            block = auto_block(m)
            want_re = len({j // block for j in bad}) * block if m % block == 0 else None
            agree = all(np.array_equal(d.cpu().numpy(), want) for d in (d_loc, d_rlc, d_item)) and set(got["rlc"]) == {0 if bad else 1} \
                and set(c for c, _ in got["loc"]) == {0 if bad else 1} and (want_re is None or set(r for _, r in got["loc"]) == {want_re})
            (loc, loc_sp), (rlc, rlc_sp), (item, item_sp) = alternate([f_loc, f_rlc, f_item], a.reps)
            read_profile(lib); lib.blsmi_set_profiling(1); f_loc(); lib.blsmi_set_profiling(0)
            prof = read_profile(lib)
            row = {"shape": "%s %dx%d" % (kind, m, k), "mode": mode, "pairs": n, "table": nq, "bad_items": len(bad), "block": block, "rechecked": got["loc"][-1][1],
                   "locate_ms": loc, "locate_spread_ms": loc_sp, "rlc_ms": rlc, "rlc_spread_ms": rlc_sp, "item_ms": item, "item_spread_ms": item_sp,
                   "rlc_minus_locate_ms": round(rlc - loc, 3), "faster_than_rlc_beyond_spreads": bool(rlc - loc > rlc_sp + loc_sp),
                   "verdicts_agree": bool(agree), "locate_profile_ms": prof}
            rows.append(row)
            say(json.dumps(row))
            if kind == "groth" and m == a.sweep_at and mode == "onebad":
                blocks = [0, 64, 256, 1024, 4096]
                fs = [lambda b=b: f_loc(b) for b in blocks]
                for f in fs:
                    f(); f()
                res = alternate(fs, a.reps)
                sweep = {"shape": row["shape"], "mode": mode, "auto_block": block,
                         "blocks": [{"block": b, "locate_ms": ms, "spread_ms": sp, "rechecked": None} for b, (ms, sp) in zip(blocks, res)]}
                for e, f in zip(sweep["blocks"], fs):
                    f(); e["rechecked"] = got["loc"][-1][1]
                best = min(sweep["blocks"][1:], key=lambda e: e["locate_ms"])
                auto = sweep["blocks"][0]
                sweep["rule_stays"] = not (auto["locate_ms"] - best["locate_ms"] > auto["spread_ms"] + best["spread_ms"])
                say("BLOCK_SWEEP " + json.dumps(sweep))
    crit = [{"shape": r["shape"], "locate_ms": r["locate_ms"], "rlc_ms": r["rlc_ms"], "item_ms": r["item_ms"], "spreads_ms": round(r["locate_spread_ms"] + r["rlc_spread_ms"], 3),
             "met": r["faster_than_rlc_beyond_spreads"]} for r in rows if r["shape"].startswith("groth") and r["mode"] == "onebad" and r["pairs"] >= 65536]
    say("CRITERION_1 " + json.dumps(crit))
    say("PPROD_RLC_LOCATE_BENCH " + json.dumps({"version": eng.version(), "reps": a.reps, "rows": rows, "block_sweep": sweep, "criterion_1": crit}))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
