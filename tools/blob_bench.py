#!/usr/bin/env python3
"""KZG blob batches (include/blsmi.h: blsmi_kzg_verify_blob_batch*, blsmi_fr_eval_batch*): what the evaluation of the blobs costs, beside the
memory floor and beside the part of the call that existed before.  Everything resident on the device, N = 2^--log2n values per blob, blob
layout (order 1), block = 0, every opening valid.  For each m four legs alternate in one process; after a warm-up of all, the median of --reps
calls and the spread (max - min), in ms, of
  (a) eval     blsmi_fr_eval_batch_dev: the three kernels together, and each from the profile segments of --kernel-reps profiled calls
  (b) copy     a device-to-device copy of the same m * N * 32 bytes: the memory floor
  (c) given    blsmi_kzg_verify_batch_dev on the same openings with y given: the part of the call that already existed
  (d) blob     blsmi_kzg_verify_blob_batch_dev
and from them (a) / (b) and (d) - (c).  The openings are made valid with the library itself: y_j = p_j(z_j) and c_j = p_j(tau) by
blsmi_fr_eval_batch_dev, q_j = (c_j - y_j) / (tau - z_j) by big integers, C_j = c_j G and pi_j = q_j G by the generator ladders; both verifying
legs must say that every item holds.  Then k_fr_mul and k_fr_inv at --lanes-at elements: the kernel's profile segment, median and spread.
Nothing is asserted: the figures are taken, not met.
usage: python tools/blob_bench.py [--reps 20] [--log2n 12] [--shapes 8,64,1024,4096] [--lanes-at 65536] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pprod_rlc_bench import R, be32, read_profile  # noqa: E402
from pprod_rlc_locate_bench import alternate  # noqa: E402

KERNELS = ("k_fr_bary_prod", "k_fr_inv", "k_fr_bary_sum")


def profiled(lib, f, names, reps):
    """{name: (median ms, spread ms)} of the profile segments of `reps` profiled calls of f"""
    ts = {k: [] for k in names}
    for _ in range(reps):
        read_profile(lib); lib.blsmi_set_profiling(1); f(); lib.blsmi_set_profiling(0)
        prof = read_profile(lib)
        for k in names:
            ts[k].append(prof.get(k, 0.0))
    return {k: (round(statistics.median(v), 4), round(max(v) - min(v), 4)) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kernel-reps", type=int, default=5)
    ap.add_argument("--log2n", type=int, default=12)
    ap.add_argument("--shapes", default="8,64,1024,4096")
    ap.add_argument("--lanes-at", type=int, default=65536)
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
    k, n = a.log2n, 1 << a.log2n
    say("%s  N = %d, reps %d (median, spread = max - min, ms; the legs alternate)" % (eng.version(), n, a.reps))
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)
    u8 = lambda b: np.frombuffer(bytes(b), dtype=np.uint8)
    ints = lambda d, cnt: [int.from_bytes(bytes(row), "big") for row in d.cpu().numpy().reshape(cnt, 32)]
    rows = []
    for m in (int(v) for v in a.shapes.split(",")):
        rng = np.random.default_rng(m + 21)
        rnd = lambda: int.from_bytes(rng.bytes(31), "big")
        tau, h0 = rnd(), rnd()
        z = [rnd() for _ in range(m)]
        gen = torch.Generator(device=dev); gen.manual_seed(m)
        d_polys = torch.randint(0, 256, (m * n, 32), dtype=torch.uint8, device=dev, generator=gen)
        d_polys[:, 0] &= 0x3f                                                    # every value below 2^254 < r
        d_polys = d_polys.view(-1)
        d_z, d_tau = t(u8(be32(z))), t(u8(be32([tau] * m)))
        d_y, d_c = (torch.zeros(32 * m, dtype=torch.uint8, device=dev) for _ in range(2))
        fr.eval_batch_dev(d_polys.data_ptr(), k, 1, d_z.data_ptr(), d_y.data_ptr(), 0, m)
        fr.eval_batch_dev(d_polys.data_ptr(), k, 1, d_tau.data_ptr(), d_c.data_ptr(), 0, m)
        y, c = ints(d_y, m), ints(d_c, m)
        q = [(cj - yj) * pow(tau - zj, -1, R) % R for cj, yj, zj in zip(c, y, z)]
        G = bytes(eng.g1_mul_generator_batch(be32([1]), 1)[0])
        srs2 = bytes(eng.g2_mul_generator_batch(be32([h0, h0 * tau]), 2)[0])
        d_G, d_srs2 = t(u8(G)), t(u8(srs2))
        d_C, d_pi = t(u8(eng.g1_mul_generator_batch(be32(c), m)[0])), t(u8(eng.g1_mul_generator_batch(be32(q), m)[0]))
        d_copy = torch.empty_like(d_polys)
        d_yy = torch.zeros(32 * m, dtype=torch.uint8, device=dev)
        d_ok_c, d_ok_d = (torch.zeros(m, dtype=torch.uint8, device=dev) for _ in range(2))
        got = {"c": [], "d": []}

        def f_eval():
            fr.eval_batch_dev(d_polys.data_ptr(), k, 1, d_z.data_ptr(), d_yy.data_ptr(), 0, m)

        def f_copy():
            d_copy.copy_(d_polys)
            torch.cuda.synchronize()

        def f_given():
            got["c"].append(kzg.verify_batch_dev(d_G.data_ptr(), d_srs2.data_ptr(), d_C.data_ptr(), d_pi.data_ptr(), d_z.data_ptr(), d_y.data_ptr(), m, d_ok_c.data_ptr()))

        def f_blob():
            got["d"].append(kzg.verify_blob_batch_dev(d_G.data_ptr(), d_srs2.data_ptr(), d_polys.data_ptr(), k, 1, d_C.data_ptr(), d_pi.data_ptr(), d_z.data_ptr(), m, d_ok_d.data_ptr()))
        legs = [f_eval, f_copy, f_given, f_blob]
        for _ in range(2):
            for f in legs:
                f()
        hold = bool(d_ok_c.cpu().numpy().all() and d_ok_d.cpu().numpy().all() and torch.equal(d_yy, d_y) and all(set(g) == {(1, 0)} for g in got.values()))
        (ev, ev_sp), (cp, cp_sp), (gv, gv_sp), (bl, bl_sp) = alternate(legs, a.reps)
        kern = profiled(lib, f_eval, KERNELS, a.kernel_reps)
        read_profile(lib); lib.blsmi_set_profiling(1); f_blob(); lib.blsmi_set_profiling(0)
        prof = read_profile(lib)
        in_call = round(sum(prof.get(x, 0.0) for x in KERNELS), 4)
        row = {"m": m, "N": n, "bytes": m * n * 32, "all_hold": hold, "eval_ms": ev, "eval_spread_ms": ev_sp, "copy_ms": cp, "copy_spread_ms": cp_sp,
               "eval_over_copy": round(ev / cp, 2), "given_ms": gv, "given_spread_ms": gv_sp, "blob_ms": bl, "blob_spread_ms": bl_sp,
               "blob_minus_given_ms": round(bl - gv, 3), "eval_kernels_ms": {x: kern[x][0] for x in KERNELS}, "eval_kernels_spread_ms": {x: kern[x][1] for x in KERNELS},
               "eval_kernels_in_blob_call_ms": in_call, "evaluation_is_the_larger_part": bool(bl - gv > gv), "blob_profile_ms": prof}
        rows.append(row)
        say(json.dumps(row))
        del d_polys, d_copy
        torch.cuda.empty_cache()
    lanes = {}
    cnt = a.lanes_at
    if cnt:
        rng = np.random.default_rng(cnt)
        d_a, d_b = (t(rng.integers(0, 256, size=32 * cnt, dtype=np.uint8)) for _ in range(2))
        d_out = torch.zeros(32 * cnt, dtype=torch.uint8, device=dev)
        calls = {"k_fr_mul": lambda: fr.mul_batch_dev(d_a.data_ptr(), d_b.data_ptr(), d_out.data_ptr(), cnt),
                 "k_fr_inv": lambda: fr.inv_batch_dev(d_a.data_ptr(), d_out.data_ptr(), cnt)}
        for name, f in calls.items():
            f()
            med, sp = profiled(lib, f, (name,), a.kernel_reps)[name]
            lanes[name] = {"median_ms": med, "spread_ms": sp}
        say("LANES at %d elements " % cnt + json.dumps(lanes))
    say("BLOB_BENCH " + json.dumps({"version": eng.version(), "reps": a.reps, "rows": rows, "lanes": lanes}))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
