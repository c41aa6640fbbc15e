#!/usr/bin/env python3
"""Groth16 batches with the public inputs folded in Fr (include/blsmi.h: blsmi_groth16_verify_batch*) against the composite a caller had
before it, everything resident on the device, block = 0.  For each shape m x nin the two alternate in one process; after warm-up of both,
the median of --reps calls and the spread (max - min), in ms, of
  new        blsmi_groth16_verify_batch_dev, with the per-stage split of one profiled call (blsmi_last_profile);
  composite  blsmi_g1_mul_batch_dev over the m * nin pre-expanded IC records (the inputs as scalars), blsmi_g1_sum_segmented_dev for
             L_j = IC_0 + the item's products, one strided device copy of the L_j into the pairs' G1 array, and
             blsmi_pairing_product_batch_rlc_locate_dev on (A_j, B_j), (alpha, -beta), (L_j, -gamma), (C_j, -delta) -- the key's G2 points
             negated beforehand, everything but the L_j laid out beforehand
with every proof valid ("valid") and with one proof whose first public input is off by one ("onebad").
Criterion: all valid, at the x 8 shapes of 16 384 proofs and more, new is faster than composite by more than the sum of the
two spreads.
usage: python tools/groth16_bench.py [--reps 20] [--shapes 16384x8,65536x8,16384x1,2048x8] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pprod_rlc_bench import R, be32, read_profile  # noqa: E402
from pprod_rlc_locate_bench import alternate, auto_block  # noqa: E402

Q = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab


def neg2(rec):
    """-Q of a 192-byte affine G2 record (x.c0, x.c1, y.c0, y.c1, big-endian)"""
    y = [(Q - int.from_bytes(rec[96 + 48 * i:144 + 48 * i], "big")) % Q for i in range(2)]
    return bytes(rec[:96]) + y[0].to_bytes(48, "big") + y[1].to_bytes(48, "big")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="16384x8,65536x8,16384x1,2048x8")
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
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)
    rows = []
    for shape in a.shapes.split(","):
        m, nin = (int(v) for v in shape.split("x"))
        rng = np.random.default_rng(m + nin)
        rnd = lambda: int.from_bytes(rng.bytes(31), "big")
        alpha, beta, gamma, delta = rnd(), rnd(), rnd(), rnd()
        ic = [rnd() for _ in range(nin + 1)]
        dinv = pow(delta, -1, R)
        x = [[rnd() for _ in range(nin)] for _ in range(m)]
        ab = [(rnd(), rnd()) for _ in range(m)]
        s1 = []
        for (pa, pb), xi in zip(ab, x):
            lsc = ic[0] + sum(v * k for v, k in zip(xi, ic[1:]))
            s1 += [pa, (pa * pb - alpha * beta - gamma * lsc) * dinv]
        vk1 = bytes(eng.g1_mul_generator_batch(be32([alpha] + ic), nin + 2)[0])
        vk2 = bytes(eng.g2_mul_generator_batch(be32([beta, gamma, delta]), 3)[0])
        pg1 = np.frombuffer(bytes(eng.g1_mul_generator_batch(be32(s1), 2 * m)[0]), dtype=np.uint8).reshape(m, 2, 96)
        pg2 = np.frombuffer(bytes(eng.g2_mul_generator_batch(be32([pb for _, pb in ab]), m)[0]), dtype=np.uint8).reshape(m, 192)
        d_vk1, d_vk2, d_pg1, d_pg2 = t(np.frombuffer(vk1, dtype=np.uint8)), t(np.frombuffer(vk2, dtype=np.uint8)), t(pg1), t(pg2)
        # the composite's resident inputs: IC_1 .. IC_nin tiled per item; the table -beta, -gamma, -delta, B_j; the pairs' G1 array with
        # A_j, alpha, (L_j: written per call), C_j; the products' buffer with IC_0 in front; the sums' index and offsets
        ic_rec = np.frombuffer(vk1, dtype=np.uint8).reshape(nin + 2, 96)
        d_icx = t(np.tile(ic_rec[2:], (m, 1)))
        tab = np.concatenate([np.frombuffer(b"".join(neg2(vk2[192 * i:192 * i + 192]) for i in range(3)), dtype=np.uint8).reshape(3, 192), pg2])
        d_tab = t(tab)
        g1a = np.zeros((m, 4, 96), dtype=np.uint8)
        g1a[:, 0], g1a[:, 1], g1a[:, 3] = pg1[:, 0], ic_rec[0], pg1[:, 1]
        d_g1a = t(g1a).view(m, 4, 96)
        d_prod = torch.zeros(96 * (1 + m * nin), dtype=torch.uint8, device=dev)
        d_prod[:96] = t(ic_rec[1])
        d_pinf = torch.zeros(1 + m * nin, dtype=torch.uint8, device=dev)
        idx = np.concatenate([np.zeros((m, 1), dtype=np.uint32), 1 + np.arange(m * nin, dtype=np.uint32).reshape(m, nin)], axis=1)
        d_idx, d_soff = t(idx), t(eng.seg_offsets([nin + 1] * m))
        d_q, d_poff = t(np.stack([3 + np.arange(m), np.zeros(m), np.ones(m), np.full(m, 2)], axis=1).astype(np.uint32)), t(eng.seg_offsets([4] * m))
        d_L, d_Linf = torch.zeros(m, 96, dtype=torch.uint8, device=dev), torch.zeros(m, dtype=torch.uint8, device=dev)
        block = auto_block(m)
        for mode in ("valid", "onebad"):
            bad = [] if mode == "valid" else [(-(-m // block) // 2) * block + 1]
            xs = [list(xi) for xi in x]
            for j in bad:
                xs[j][0] += 1
            d_in = t(np.frombuffer(be32([v for xi in xs for v in xi]) or bytes(8), dtype=np.uint8))
            d_new, d_old = (torch.zeros(m, dtype=torch.uint8, device=dev) for _ in range(2))
            got = {"new": [], "old": []}

            def f_new():
                got["new"].append(eng.groth16_verify_batch_dev(d_vk1.data_ptr(), d_vk2.data_ptr(), nin, d_pg1.data_ptr(), d_pg2.data_ptr(), d_in.data_ptr(), m, d_new.data_ptr()))

            def f_old():
                if nin:
                    eng.mul_batch_dev("g1", d_icx.data_ptr(), d_in.data_ptr(), d_prod.data_ptr() + 96, d_pinf.data_ptr() + 1, m * nin)
                eng.sum_segmented_dev("g1", d_prod.data_ptr(), d_pinf.data_ptr(), 1 + m * nin, d_idx.data_ptr(), d_soff.data_ptr(), m, d_L.data_ptr(), d_Linf.data_ptr())
                d_g1a[:, 2] = d_L
                torch.cuda.synchronize()
                got["old"].append(eng.pairing_product_batch_rlc_locate_dev(d_g1a.data_ptr(), d_tab.data_ptr(), 3 + m, d_q.data_ptr(), 4 * m, d_poff.data_ptr(), m, d_old.data_ptr()))
            for _ in range(2):
                f_new(); f_old()
            want = np.ones(m, dtype=np.uint8); want[bad] = 0
            want_re = len(bad) * block if m % block == 0 else None
            agree = all(np.array_equal(d.cpu().numpy(), want) for d in (d_new, d_old)) and all(set(c for c, _ in g) == {0 if bad else 1} for g in got.values()) \
                and (want_re is None or all(set(r for _, r in g) == {want_re} for g in got.values()))
            (new, new_sp), (old, old_sp) = alternate([f_new, f_old], a.reps)
            read_profile(lib); lib.blsmi_set_profiling(1); f_new(); lib.blsmi_set_profiling(0)
            prof = read_profile(lib)
            row = {"shape": "%dx%d" % (m, nin), "mode": mode, "block": block, "rechecked": got["new"][-1][1], "new_ms": new, "new_spread_ms": new_sp,
                   "composite_ms": old, "composite_spread_ms": old_sp, "composite_minus_new_ms": round(old - new, 3),
                   "faster_beyond_spreads": bool(old - new > old_sp + new_sp), "verdicts_agree": bool(agree), "fold_ms": prof.get("k_fr_wsum_u64"), "new_profile_ms": prof}
            rows.append(row)
            say(json.dumps(row))
    crit = [{"shape": r["shape"], "new_ms": r["new_ms"], "composite_ms": r["composite_ms"], "spreads_ms": round(r["new_spread_ms"] + r["composite_spread_ms"], 3),
             "met": r["faster_beyond_spreads"]} for r in rows if r["mode"] == "valid" and r["shape"].endswith("x8") and int(r["shape"].split("x")[0]) >= 16384]
    say("CRITERION " + json.dumps(crit))
    say("GROTH16_BENCH " + json.dumps({"version": eng.version(), "reps": a.reps, "rows": rows, "criterion": crit}))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
