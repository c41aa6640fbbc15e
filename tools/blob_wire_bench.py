#!/usr/bin/env python3
"""KZG blob batches from wire bytes (include/blsmi.h: blsmi_kzg_blob_challenge_batch*, blsmi_kzg_verify_blob_batch_wire*): what the
Fiat-Shamir challenge costs in either form of its kernel, beside the memory floor and beside the host's hash, and what the wire call adds to
the call that existed before.  Everything resident on the device, N = 2^--log2n values per blob, block = 0, every item valid.  For each m, after
a warm-up of all legs, three alternations in one process -- (A) with (B) alone, as the criterion asks; (c), (h1), (h16); (g), (w), (s) -- and
of each leg the median of --reps calls and the spread (max - min), in ms:
  (A) lane     blsmi_debug_kzg_blob_challenge_form_dev, form 0: k_kzg_fs_lane
  (B) split    ... form 1: k_kzg_fs_split
  (c) copy     a device-to-device copy of the same m * N * 32 bytes: the memory floor
  (h1) host 1  hashlib.sha256 over the same m messages on one host thread, the reduction mod r included
  (h16) host 16  the same on 16 threads (hashlib releases the interpreter lock while it hashes)
  (g) given    blsmi_kzg_verify_blob_batch_dev given z and the affine points: the call that existed before
  (w) wire     blsmi_kzg_verify_blob_batch_wire_dev: the decompression beside the hash, on the lease's side stream
  (s) serial   blsmi_debug_kzg_verify_blob_batch_wire_dev_serial: the decompression on the main stream
and from them the criterion for the two forms (B stays only if A - B exceeds the sum of the two spreads), (B) / (c), the host's legs over
(B), (w) - (g) and (s) - (w).  The items are made valid with the library itself: c_j = p_j(tau) by blsmi_fr_eval_batch_dev, C_j = c_j G by
the generator ladder, its compression, z_j by the challenge (the first --check of them held against hashlib), y_j = p_j(z_j), q_j = (c_j -
y_j) / (tau - z_j) by big integers, pi_j = q_j G; all three verifying legs must say that every item holds.  Nothing is asserted: the figures
are taken, not met.
usage: python tools/blob_wire_bench.py [--reps 20] [--log2n 12] [--shapes 8,64,1024,4096] [--out FILE]"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pprod_rlc_bench import R, be32, read_profile  # noqa: E402
from pprod_rlc_locate_bench import alternate  # noqa: E402

PREFIX = b"FSBLOBVERIFY_V1_"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--log2n", type=int, default=12)
    ap.add_argument("--shapes", default="8,64,1024,4096")
    ap.add_argument("--check", type=int, default=8)
    ap.add_argument("--threads", type=int, default=16)
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
    head = PREFIX + n.to_bytes(16, "big")
    pool = ThreadPoolExecutor(a.threads)
    rows = []
    for m in (int(v) for v in a.shapes.split(",")):
        rng = np.random.default_rng(m + 23)
        rnd = lambda: int.from_bytes(rng.bytes(31), "big")
        tau, h0 = rnd(), rnd()
        gen = torch.Generator(device=dev); gen.manual_seed(m)
        d_polys = torch.randint(0, 256, (m * n, 32), dtype=torch.uint8, device=dev, generator=gen)
        d_polys[:, 0] &= 0x3f                                                    # every value below 2^254 < r
        d_polys = d_polys.view(-1)
        d_tau = t(u8(be32([tau] * m)))
        d_y, d_c, d_z, d_zz = (torch.zeros(32 * m, dtype=torch.uint8, device=dev) for _ in range(4))
        fr.eval_batch_dev(d_polys.data_ptr(), k, 1, d_tau.data_ptr(), d_c.data_ptr(), 0, m)
        c = ints(d_c, m)
        G = bytes(eng.g1_mul_generator_batch(be32([1]), 1)[0])
        srs2 = bytes(eng.g2_mul_generator_batch(be32([h0, h0 * tau]), 2)[0])
        C_aff = eng.g1_mul_generator_batch(be32(c), m)[0]
        c48 = np.ascontiguousarray(eng.g1_compress_batch(C_aff, m))
        d_c48 = t(c48)
        kzg.blob_challenge_batch_dev(d_polys.data_ptr(), k, d_c48.data_ptr(), d_z.data_ptr(), m)
        z = ints(d_z, m)
        blobs = d_polys.cpu().numpy().reshape(m, 32 * n)                         # the host's copy: what its hash reads
        c48_rows = c48.reshape(m, 48)

        def host_z(j):
            return int.from_bytes(hashlib.sha256(head + blobs[j].tobytes() + c48_rows[j].tobytes()).digest(), "big") % R
        z_ok = all(host_z(j) == z[j] for j in range(min(m, a.check)))
        fr.eval_batch_dev(d_polys.data_ptr(), k, 1, d_z.data_ptr(), d_y.data_ptr(), 0, m)
        y = ints(d_y, m)
        q = [(cj - yj) * pow(tau - zj, -1, R) % R for cj, yj, zj in zip(c, y, z)]
        P_aff = eng.g1_mul_generator_batch(be32(q), m)[0]
        d_G, d_srs2 = t(u8(G)), t(u8(srs2))
        d_C, d_pi = t(u8(C_aff)), t(u8(P_aff))
        d_p48 = t(np.ascontiguousarray(eng.g1_compress_batch(P_aff, m)))
        d_copy = torch.empty_like(d_polys)
        d_ok_g, d_ok_w, d_ok_s, d_st = (torch.zeros(m, dtype=torch.uint8, device=dev) for _ in range(4))
        got = {"g": [], "w": [], "s": []}
        host = {}

        def form(which):
            def f():
                eng._call("blsmi_debug_kzg_blob_challenge_form_dev", d_polys.data_ptr(), k, d_c48.data_ptr(), d_zz.data_ptr(), m, which, 0)
            return f

        def f_copy():
            d_copy.copy_(d_polys)
            torch.cuda.synchronize()

        def f_host1():
            host["one"] = [host_z(j) for j in range(m)]

        def f_host16():
            host["many"] = list(pool.map(host_z, range(m)))

        def f_given():
            got["g"].append(kzg.verify_blob_batch_dev(d_G.data_ptr(), d_srs2.data_ptr(), d_polys.data_ptr(), k, 1, d_C.data_ptr(), d_pi.data_ptr(), d_z.data_ptr(), m, d_ok_g.data_ptr()))

        def f_wire():
            got["w"].append(kzg.verify_blob_batch_wire_dev(d_G.data_ptr(), d_srs2.data_ptr(), d_polys.data_ptr(), k, d_c48.data_ptr(), d_p48.data_ptr(), m, d_ok_w.data_ptr(), d_status=d_st.data_ptr()))

        def f_serial():
            comb, nre = C.c_int(0), C.c_size_t(0)
            eng._call("blsmi_debug_kzg_verify_blob_batch_wire_dev_serial", d_G.data_ptr(), d_srs2.data_ptr(), d_polys.data_ptr(), k, d_c48.data_ptr(), d_p48.data_ptr(), m,
                      None, 0, d_ok_s.data_ptr(), 0, C.byref(comb), C.byref(nre), 0)
            got["s"].append((comb.value, nre.value))
        legs = [form(0), form(1), f_copy, f_host1, f_host16, f_given, f_wire, f_serial]
        forms_agree = True
        for _ in range(2):
            for f in legs:
                f()
                if f in legs[:2]:
                    forms_agree = forms_agree and torch.equal(d_zz, d_z)
        hold = bool(d_ok_g.cpu().numpy().all() and d_ok_w.cpu().numpy().all() and d_ok_s.cpu().numpy().all() and not d_st.cpu().numpy().any()
                    and all(set(g) == {(1, 0)} for g in got.values()) and host["one"] == z and host["many"] == z and z_ok and forms_agree)
        # three alternations of their own: the two forms (the criterion: nothing else between their samples), the challenge's yardsticks,
        # the three verifying calls
        (la, la_sp), (sp, sp_sp) = alternate(legs[:2], a.reps)
        (cp, cp_sp), (h1, h1_sp), (h16, h16_sp) = alternate(legs[2:5], a.reps)
        (gv, gv_sp), (wr, wr_sp), (se, se_sp) = alternate(legs[5:], a.reps)
        read_profile(lib); lib.blsmi_set_profiling(1); f_wire(); lib.blsmi_set_profiling(0)
        prof = read_profile(lib)
        row = {"m": m, "N": n, "bytes": m * n * 32, "all_hold": hold,
               "lane_ms": la, "lane_spread_ms": la_sp, "split_ms": sp, "split_spread_ms": sp_sp,
               "lane_minus_split_ms": round(la - sp, 3), "sum_of_spreads_ms": round(la_sp + sp_sp, 3), "split_beats_lane_by_more": bool(la - sp > la_sp + sp_sp),
               "copy_ms": cp, "copy_spread_ms": cp_sp, "split_over_copy": round(sp / cp, 1),
               "host1_ms": h1, "host1_spread_ms": h1_sp, "host16_ms": h16, "host16_spread_ms": h16_sp,
               "host1_over_split": round(h1 / sp, 2), "host16_over_split": round(h16 / sp, 2),
               "given_ms": gv, "given_spread_ms": gv_sp, "wire_ms": wr, "wire_spread_ms": wr_sp, "wire_minus_given_ms": round(wr - gv, 3),
               "serial_ms": se, "serial_spread_ms": se_sp, "serial_minus_wire_ms": round(se - wr, 3), "wire_profile_ms": prof}
        rows.append(row)
        say(json.dumps(row))
        del d_polys, d_copy, blobs
        torch.cuda.empty_cache()
    say("BLOB_WIRE_BENCH " + json.dumps({"version": eng.version(), "reps": a.reps, "threads": a.threads, "rows": rows}))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
