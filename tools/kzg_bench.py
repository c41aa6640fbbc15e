#!/usr/bin/env python3
"""KZG batches with the values folded in Fr (include/blsmi.h: blsmi_kzg_verify_batch*) against the composite a caller had before it,
everything resident on the device, block = 0.  For each m the two alternate in one process; after warm-up of both, the median of --reps
calls and the spread (max - min), in ms, of
  new        blsmi_kzg_verify_batch_dev, with the per-stage split of one profiled call (blsmi_last_profile);
  composite  blsmi_g1_mul_batch_dev for z_j pi_j, blsmi_g1_mul_batch_dev with d_pts = NULL for (r - y_j) G (the negated values resident
             beforehand), blsmi_g1_sum_segmented_dev over the three points C_j, z_j pi_j, (r - y_j) G, one strided device copy of the P_j
             into the pairs' G1 array, and blsmi_pairing_product_batch_rlc_locate_dev on (P_j, H), (pi_j, -tau H) -- tau H negated
             beforehand, everything but the P_j laid out beforehand
with every opening valid ("valid") and with one opening whose value is off by one ("onebad").  Then k_g1_mul_add_glv against k_g1_mul_glv at
--kernel-at items: the kernel's profile segment of one call each, median of three and spread.
Criterion: all valid, at 16 384 and at 65 536 openings, new is faster than composite by more than the sum of the two spreads.
usage: python tools/kzg_bench.py [--reps 20] [--shapes 2048,16384,65536] [--kernel-at 65536] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from groth16_bench import neg2  # noqa: E402
from pprod_rlc_bench import R, be32, read_profile  # noqa: E402
from pprod_rlc_locate_bench import alternate, auto_block  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="2048,16384,65536")
    ap.add_argument("--kernel-at", type=int, default=65536)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from bls_amd import _native, engine as eng, kzg
    eng.init(0)
    lib = _native.load()
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("%s  reps %d (median, spread = max - min, ms; the calls alternate)" % (eng.version(), a.reps))
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)
    u8 = lambda b: np.frombuffer(bytes(b), dtype=np.uint8)
    rows = []
    for m in (int(v) for v in a.shapes.split(",")):
        rng = np.random.default_rng(m + 20)
        rnd = lambda: int.from_bytes(rng.bytes(31), "big")
        tau, h0 = rnd(), rnd()
        c, z, q = ([rnd() for _ in range(m)] for _ in range(3))
        y = [(cj - qj * (tau - zj)) % R for cj, zj, qj in zip(c, z, q)]
        G = bytes(eng.g1_mul_generator_batch(be32([1]), 1)[0])
        srs2 = bytes(eng.g2_mul_generator_batch(be32([h0, h0 * tau]), 2)[0])
        C = u8(eng.g1_mul_generator_batch(be32(c), m)[0]).reshape(m, 96)
        pi = u8(eng.g1_mul_generator_batch(be32(q), m)[0]).reshape(m, 96)
        d_G, d_srs2, d_C, d_pi, d_z = t(u8(G)), t(u8(srs2)), t(C), t(pi), t(u8(be32(z)))
        # the composite's resident inputs: the three points of every item in one array (C_j; z_j pi_j and (r - y_j) G written per call) with
        # its index and offsets; the table H, -tau H; the pairs' G1 array with (P_j: written per call), pi_j
        d_pts = torch.zeros(3 * m, 96, dtype=torch.uint8, device=dev)
        d_pts[:m] = d_C.view(m, 96)
        d_pinf = torch.zeros(3 * m, dtype=torch.uint8, device=dev)
        idx = np.stack([np.arange(m), m + np.arange(m), 2 * m + np.arange(m)], axis=1).astype(np.uint32)
        d_idx, d_soff = t(idx), t(eng.seg_offsets([3] * m))
        d_tab = t(u8(srs2[:192] + neg2(srs2[192:])))
        g1a = np.zeros((m, 2, 96), dtype=np.uint8)
        g1a[:, 1] = pi
        d_g1a = t(g1a).view(m, 2, 96)
        d_q, d_poff = t(np.tile(np.array([0, 1], dtype=np.uint32), m)), t(eng.seg_offsets([2] * m))
        d_P, d_Pinf = torch.zeros(m, 96, dtype=torch.uint8, device=dev), torch.zeros(m, dtype=torch.uint8, device=dev)
        block = auto_block(m)
        for mode in ("valid", "onebad"):
            bad = [] if mode == "valid" else [(-(-m // block) // 2) * block + 1]
            ys = list(y)
            for j in bad:
                ys[j] = (ys[j] + 1) % R
            d_y, d_negy = t(u8(be32(ys))), t(u8(be32([R - v for v in ys])))
            d_new, d_old = (torch.zeros(m, dtype=torch.uint8, device=dev) for _ in range(2))
            got = {"new": [], "old": []}

            def f_new():
                got["new"].append(kzg.verify_batch_dev(d_G.data_ptr(), d_srs2.data_ptr(), d_C.data_ptr(), d_pi.data_ptr(), d_z.data_ptr(), d_y.data_ptr(), m, d_new.data_ptr()))

            def f_old():
                eng.mul_batch_dev("g1", d_pi.data_ptr(), d_z.data_ptr(), d_pts.data_ptr() + 96 * m, d_pinf.data_ptr() + m, m)
                eng.mul_batch_dev("g1", 0, d_negy.data_ptr(), d_pts.data_ptr() + 192 * m, d_pinf.data_ptr() + 2 * m, m)
                eng.sum_segmented_dev("g1", d_pts.data_ptr(), d_pinf.data_ptr(), 3 * m, d_idx.data_ptr(), d_soff.data_ptr(), m, d_P.data_ptr(), d_Pinf.data_ptr())
                d_g1a[:, 0] = d_P
                torch.cuda.synchronize()
                got["old"].append(eng.pairing_product_batch_rlc_locate_dev(d_g1a.data_ptr(), d_tab.data_ptr(), 2, d_q.data_ptr(), 2 * m, d_poff.data_ptr(), m, d_old.data_ptr()))
            for _ in range(2):
                f_new(); f_old()
            want = np.ones(m, dtype=np.uint8); want[bad] = 0
            want_re = len(bad) * block if m % block == 0 else None
            agree = all(np.array_equal(d.cpu().numpy(), want) for d in (d_new, d_old)) and all(set(cb for cb, _ in g) == {0 if bad else 1} for g in got.values()) \
                and (want_re is None or all(set(r for _, r in g) == {want_re} for g in got.values()))
            (new, new_sp), (old, old_sp) = alternate([f_new, f_old], a.reps)
            read_profile(lib); lib.blsmi_set_profiling(1); f_new(); lib.blsmi_set_profiling(0)
            prof = read_profile(lib)
            row = {"m": m, "mode": mode, "block": block, "rechecked": got["new"][-1][1], "new_ms": new, "new_spread_ms": new_sp,
                   "composite_ms": old, "composite_spread_ms": old_sp, "composite_minus_new_ms": round(old - new, 3),
                   "faster_beyond_spreads": bool(old - new > old_sp + new_sp), "verdicts_agree": bool(agree), "lift_ms": prof.get("k_g1_mul_add_glv"),
                   "fold_ms": prof.get("k_fr_wsum_u64"), "new_profile_ms": prof}
            rows.append(row)
            say(json.dumps(row))
    crit = [{"m": r["m"], "new_ms": r["new_ms"], "composite_ms": r["composite_ms"], "spreads_ms": round(r["new_spread_ms"] + r["composite_spread_ms"], 3),
             "met": r["faster_beyond_spreads"]} for r in rows if r["mode"] == "valid" and r["m"] >= 16384]
    say("CRITERION " + json.dumps(crit))
    # the lift's kernel against the ladder's, one launch each over the same multiplicands and scalars
    n = a.kernel_at
    kern = {}
    if n:
        rng = np.random.default_rng(n)
        sc = [int.from_bytes(rng.bytes(31), "big") for _ in range(2 * n)]
        pts = u8(eng.g1_mul_generator_batch(be32(sc), 2 * n)[0])
        d_a, d_b = t(pts[:96 * n]), t(pts[96 * n:])
        d_k = t(u8(be32([int.from_bytes(rng.bytes(32), "big") for _ in range(n)])))
        d_out, d_inf = torch.zeros(96 * n, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
        calls = {"k_g1_mul_add_glv": lambda: kzg.g1_mul_add_batch_dev(d_a.data_ptr(), 96, d_b.data_ptr(), 96, d_k.data_ptr(), d_out.data_ptr(), d_inf.data_ptr(), n),
                 "k_g1_mul_glv": lambda: eng.mul_batch_dev("g1", d_b.data_ptr(), d_k.data_ptr(), d_out.data_ptr(), d_inf.data_ptr(), n)}
        for f in calls.values():
            f()
        ts = {k: [] for k in calls}
        for _ in range(3):
            for k, f in calls.items():
                read_profile(lib); lib.blsmi_set_profiling(1); f(); lib.blsmi_set_profiling(0)
                ts[k].append(read_profile(lib).get(k))
        kern = {k: {"median_ms": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4)} for k, v in ts.items()}
        say("KERNELS at %d items " % n + json.dumps(kern))
    say("KZG_BENCH " + json.dumps({"version": eng.version(), "reps": a.reps, "rows": rows, "criterion": crit, "kernels": kern}))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
