#!/usr/bin/env python3
"""Times of the wire format <-> in-memory point conversions (blsmi 0.15), per n (default 4 096 and 65 536) on n subgroup points
(sk_i * generator, computed on the device; in-memory records under a random z unless --z-one):

(a) call time from host buffers (wall clock around the library call, time.perf_counter):
    one_call_g?   blsmi_g?_compress_batch_jac
    two_calls_g?  blsmi_g?_jac_to_affine_batch, then blsmi_g?_compress_batch: the route before 0.15, in the same process
(b) kernel time, from the library's own profile (blsmi_set_profiling / blsmi_last_profile: HIP events around each kernel on the launch stream):
    k_g?_compress_jac                           blsmi_g?_compress_batch_jac
    k_g?_decompress_jac against k_g?_decompress blsmi_g?_decompress_batch[_jac], check = 1, latency threshold 0 so that both run the subgroup
                                                test inside the kernel
Each is run --reps times (default 3) after one warm-up, the kinds interleaved; one JSON line per (n, kind) with the times, their median and
spread (max - min).  A kernel named <kernel>_pair is counted as <kernel>: the lane-pair G2 compression kernel was measured with this tool
against the one-lane kernel (which a BLSMI_LAYOUT=single process then ran) before it was dropped (profiles/wire_jac.log).

    python tools/wire_jac_bench.py [--sizes 4096,65536] [--reps 3] [--z-one] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bls_amd import engine  # noqa: E402

Q = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab


def profile(lib, buf):
    lib.blsmi_last_profile(buf, ctypes.c_size_t(len(buf)))
    out = {}
    for item in buf.value.decode().split(";"):
        if "=" in item:
            k, v = item.rsplit("=", 1)
            out[k.strip()] = out.get(k.strip(), 0.0) + float(v)
    return out


def rescale(jac, group, rng):
    """the same points under a z that is not 1: (x z^2, y z^3, z) with z a small Fq value per point, in host big integers (Montgomery limbs
    stay Montgomery limbs under a multiplication by a plain integer)"""
    nc = group
    out = bytearray(jac)
    step = 144 * nc
    for i in range(len(jac) // step):
        z = int(rng.integers(2, 1 << 30))
        for e, k in [(c, 2) for c in range(nc)] + [(nc + c, 3) for c in range(nc)] + [(2 * nc, 1)]:
            o = i * step + 48 * e
            v = int.from_bytes(jac[o:o + 48], "little") * pow(z, k, Q) % Q
            out[o:o + 48] = v.to_bytes(48, "little")
    return bytes(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,65536")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--z-one", action="store_true", help="leave z = 1: every wave takes the shortcut that skips the inversion")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    engine.init(0)
    lib = engine._lib()
    buf = ctypes.create_string_buffer(1 << 16)
    rng = np.random.default_rng(20261)
    lines = []
    for n in [int(s) for s in a.sizes.split(",")]:
        sk = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        sk[:, 0] &= 0x3f                                                      # below r
        sk = sk.tobytes()
        work = []
        for group, g in ((1, "g1"), (2, "g2")):
            jac = getattr(engine, g + "_mul_generator_batch_jac")(sk, n).tobytes()
            if not a.z_one:
                jac = rescale(jac, group, rng)
            one = getattr(engine, g + "_compress_batch_jac")
            to_affine, compress = getattr(engine, g + "_jac_to_affine_batch"), getattr(engine, g + "_compress_batch")
            comp = one(jac, n).tobytes()

            def two_calls(jac=jac, to_affine=to_affine, compress=compress):
                pts, inf = to_affine(jac, n)
                return compress(pts, n, inf.astype(np.uint8))
            assert two_calls().tobytes() == comp
            work.append(("one_call_" + g, "k_%s_compress_jac" % g, lambda jac=jac, one=one: one(jac, n)))
            work.append(("two_calls_" + g, None, two_calls))
            work.append((None, "k_%s_decompress_jac" % g, lambda g=g, comp=comp: getattr(engine, g + "_decompress_batch_jac")(comp, n, 1)))
            work.append((None, "k_%s_decompress" % g, lambda g=g, comp=comp: getattr(engine, g + "_decompress_batch")(comp, n, 1)))
        engine.set_latency_threshold(0)
        wall, kern = {}, {}
        try:
            for rep in range(a.reps + 1):                                     # (rep 0: warm-up)
                for timed in (True, False):                                   # wall clock without the profile's events, then the kernels
                    lib.blsmi_set_profiling(0 if timed else 1)
                    for call_name, kernel, call in work:
                        if timed and call_name is None or not timed and kernel is None:
                            continue
                        t0 = time.perf_counter()
                        call()
                        dt = (time.perf_counter() - t0) * 1e3
                        if not rep:
                            continue
                        if timed:
                            wall.setdefault(call_name, []).append(dt)
                        else:
                            prof = profile(lib, buf)
                            hit = [k for k in prof if k == kernel or k == kernel + "_pair"]
                            assert len(hit) == 1, (kernel, prof)
                            kern.setdefault(hit[0], []).append(prof[hit[0]])
        finally:
            lib.blsmi_set_profiling(0)
            engine.set_latency_threshold(8192)
        for kind, table in (("call", wall), ("kernel", kern)):
            for k, v in table.items():
                lines.append(json.dumps({"n": n, kind: k, "layout": os.environ.get("BLSMI_LAYOUT", "default"), "z": "one" if a.z_one else "random",
                                         "ms": [round(x, 4) for x in v], "median_ms": round(float(np.median(v)), 4), "spread_ms": round(max(v) - min(v), 4)}))
                print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
