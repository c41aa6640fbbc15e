#!/usr/bin/env python3
"""KZG cell batches (include/blsmi.h: blsmi_kzg_verify_cell_batch*, blsmi_fr_coset_interp_batch*): what the interpolation of the cells, the
n-column fold and the B * n key ladders cost, beside the memory floor and beside the pairing side that existed before.  Everything resident
on the device, n = 2^--log2n values per cell, bit-reversed order (1), the shifts of an EIP-7594 extended blob in turn, block = 0.  For each m
five legs alternate in one process; after a warm-up of all, the median of --reps calls and the spread (max - min), in ms, of
  (a) interp   blsmi_fr_coset_interp_batch_dev: the two kernels together, and each from the profile segments of --kernel-reps profiled calls
  (b) copy     a device-to-device copy of the same m * n * 32 bytes: the memory floor
  (c) point    blsmi_kzg_verify_batch_dev on m openings over the same key points (z_j = h_j^n, y_j = I_j(tau), tau H := [tau^n] H): the
               pairing side without the n-column fold, the floor this call cannot go under
  (d) cell     blsmi_kzg_verify_cell_batch_dev, every cell valid
  (e) spoiled  the same with one value of one cell incremented
and from them (a) / (b), (d) - (c) -- split by the profile segments of one profiled call of (d) and of (c) -- and (e) - (d).  The cells are
made valid with the library itself: random values, their interpolants by blsmi_fr_coset_interp_batch_dev, I_j(tau) by big integers, a random
q_j, c_j = I_j(tau) + q_j (tau^n - h_j^n), C_j = c_j G and pi_j = q_j G by the generator ladders; the verifying legs must say that every item
holds, the spoiled leg that exactly one does not.  Nothing is asserted: the figures are taken, not met.
usage: python tools/cell_bench.py [--reps 20] [--log2n 6] [--shapes 128,1024,8192,16384] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from blob_bench import profiled  # noqa: E402
from pprod_rlc_bench import R, be32, read_profile  # noqa: E402
from pprod_rlc_locate_bench import alternate  # noqa: E402

KERNELS = ("k_fr_inv", "k_fr_coset_interp")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kernel-reps", type=int, default=5)
    ap.add_argument("--log2n", type=int, default=6)
    ap.add_argument("--shapes", default="128,1024,8192,16384")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from bls_amd import _native, engine as eng, fr, kzg
    eng.init(0)
    lib = _native.load()
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    l, n = a.log2n, 1 << a.log2n
    say("%s  n = %d, reps %d (median, spread = max - min, ms; the legs alternate)" % (eng.version(), n, a.reps))
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)
    u8 = lambda b: np.frombuffer(bytes(b), dtype=np.uint8)
    ints = lambda d, cnt: [int.from_bytes(bytes(row), "big") for row in d.cpu().numpy().reshape(cnt, 32)]
    hs = [int.from_bytes(bytes(r), "big") for r in kzg.cell_shifts(7, l)]
    rows = []
    for m in (int(v) for v in a.shapes.split(",")):
        rng = np.random.default_rng(m + 22)
        rnd = lambda: int.from_bytes(rng.bytes(31), "big")
        tau, h0 = rnd(), rnd()
        h = [hs[j % len(hs)] for j in range(m)]
        gen = torch.Generator(device=dev); gen.manual_seed(m)
        d_vals = torch.randint(0, 256, (m * n, 32), dtype=torch.uint8, device=dev, generator=gen)
        d_vals[:, 0] &= 0x3f                                                     # every value below 2^254 < r
        d_vals = d_vals.view(-1)
        d_h = t(u8(be32(h)))
        d_co = torch.zeros(32 * n * m, dtype=torch.uint8, device=dev)
        d_sp = torch.zeros(32 * m, dtype=torch.uint8, device=dev)
        fr.coset_interp_batch_dev(d_vals.data_ptr(), l, 1, d_h.data_ptr(), d_co.data_ptr(), d_sp.data_ptr(), 0, m)
        co, hn = ints(d_co, m * n), ints(d_sp, m)
        tp = [pow(tau, i, R) for i in range(n + 1)]
        it = [sum(c * p for c, p in zip(co[n * j:n * j + n], tp)) % R for j in range(m)]
        q = [rnd() for _ in range(m)]
        c = [(it[j] + q[j] * (tp[n] - hn[j])) % R for j in range(m)]
        srs1 = bytes(eng.g1_mul_generator_batch(be32(tp[:n]), n)[0])
        srs2 = bytes(eng.g2_mul_generator_batch(be32([h0, h0 * tp[n]]), 2)[0])
        d_srs1, d_srs2 = t(u8(srs1)), t(u8(srs2))
        d_C, d_pi = t(u8(eng.g1_mul_generator_batch(be32(c), m)[0])), t(u8(eng.g1_mul_generator_batch(be32(q), m)[0]))
        d_y = t(u8(be32(it)))
        d_bad = d_vals.clone()
        d_bad[32 * ((m // 2) * n + 5) + 31] ^= 1                                 # one value of cell m / 2 moved by one
        d_copy = torch.empty_like(d_vals)
        d_cc = torch.zeros_like(d_co)
        d_ok_c, d_ok_d, d_ok_e = (torch.zeros(m, dtype=torch.uint8, device=dev) for _ in range(3))
        got = {"c": [], "d": [], "e": []}

        def f_interp():
            fr.coset_interp_batch_dev(d_vals.data_ptr(), l, 1, d_h.data_ptr(), d_cc.data_ptr(), 0, 0, m)

        def f_copy():
            d_copy.copy_(d_vals)
            torch.cuda.synchronize()

        def f_point():
            got["c"].append(kzg.verify_batch_dev(d_srs1.data_ptr(), d_srs2.data_ptr(), d_C.data_ptr(), d_pi.data_ptr(), d_sp.data_ptr(), d_y.data_ptr(), m, d_ok_c.data_ptr()))

        def f_cell():
            got["d"].append(kzg.verify_cell_batch_dev(d_srs1.data_ptr(), d_srs2.data_ptr(), d_vals.data_ptr(), l, 1, d_h.data_ptr(), d_C.data_ptr(), d_pi.data_ptr(), m, d_ok_d.data_ptr()))

        def f_spoiled():
            got["e"].append(kzg.verify_cell_batch_dev(d_srs1.data_ptr(), d_srs2.data_ptr(), d_bad.data_ptr(), l, 1, d_h.data_ptr(), d_C.data_ptr(), d_pi.data_ptr(), m, d_ok_e.data_ptr()))
        legs = [f_interp, f_copy, f_point, f_cell, f_spoiled]
        for _ in range(2):
            for f in legs:
                f()
        ok_e = d_ok_e.cpu().numpy()
        hold = bool(d_ok_c.cpu().numpy().all() and d_ok_d.cpu().numpy().all() and torch.equal(d_cc, d_co) and all(set(got[k]) == {(1, 0)} for k in "cd")
                    and int(ok_e.sum()) == m - 1 and ok_e[m // 2] == 0 and all(g[0] == 0 for g in got["e"]))
        nre = got["e"][0][1]
        (iv, iv_sp), (cp, cp_sp), (pt, pt_sp), (ce, ce_sp), (sp, sp_sp) = alternate(legs, a.reps)
        kern = profiled(lib, f_interp, KERNELS, a.kernel_reps)
        prof = {}
        for name, f in (("point", f_point), ("cell", f_cell)):
            read_profile(lib); lib.blsmi_set_profiling(1); f(); lib.blsmi_set_profiling(0)
            prof[name] = read_profile(lib)
        added = {k: round(prof["cell"].get(k, 0.0) - prof["point"].get(k, 0.0), 4) for k in sorted(set(prof["cell"]) | set(prof["point"]))}
        blocks = -(-m // max(64, -(-m // 256)))
        row = {"m": m, "n": n, "bytes": m * n * 32, "blocks": blocks, "key_ladders": blocks * n, "all_as_expected": hold, "interp_ms": iv, "interp_spread_ms": iv_sp,
               "copy_ms": cp, "copy_spread_ms": cp_sp, "interp_over_copy": round(iv / cp, 2), "point_ms": pt, "point_spread_ms": pt_sp, "cell_ms": ce, "cell_spread_ms": ce_sp,
               "cell_minus_point_ms": round(ce - pt, 3), "spoiled_ms": sp, "spoiled_spread_ms": sp_sp, "spoiled_minus_cell_ms": round(sp - ce, 3), "spoiled_rechecked": nre,
               "interp_kernels_ms": {x: kern[x][0] for x in KERNELS}, "interp_kernels_spread_ms": {x: kern[x][1] for x in KERNELS},
               "cell_segments_minus_point_segments_ms": {k: v for k, v in added.items() if v}, "cell_profile_ms": prof["cell"], "point_profile_ms": prof["point"]}
        rows.append(row)
        say(json.dumps(row))
        del d_vals, d_copy, d_bad, d_co, d_cc
        torch.cuda.empty_cache()
    say("CELL_BENCH " + json.dumps({"version": eng.version(), "reps": a.reps, "rows": rows}))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
