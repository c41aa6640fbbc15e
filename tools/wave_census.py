#!/usr/bin/env python3
"""Where and when the waves of the lane-pair pairing kernels ran: python tools/wave_census.py ab/libblsmi_NAME.so [n]

NAME is a diagnostic build of the library (never the product build):
    tools/build_variant.sh census1 k_pairing_pair.hip,k_fe_pair.hip "-DBLSMI_WAVE_CENSUS"
    tools/build_variant.sh census0 k_pairing_pair.hip,k_fe_pair.hip "-DBLSMI_WAVE_CENSUS -DBLSMI_PAIR_YIELD=0"
in which k_miller1h_pair and k_final_exp_pair leave one record per wave (pair_kernels.inc: WaveCensus): HW_ID / XCC_ID and the
constant-rate clock (s_memrealtime, 100 MHz) at entry and at exit, in a __device__ array of their translation unit (read back through
blsmi_census_read_miller / _fe, which only such a build exports).  This tool runs one
n-pairing call (default 65 536: two waves on each of the 1 024 SIMDs), reads the arrays, groups the waves by (XCC, SE, SH, CU, SIMD) and
prints per kernel when the first and the second wave of a SIMD left, as fractions of the kernel's span (first entry to last exit)."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WORDS, WAVES = 4, 4096


def read_records(lib, name):
    out = np.zeros(WAVES * WORDS, dtype=np.uint64)
    rc = getattr(lib, name)(out.ctypes.data_as(C.c_void_p))              # hipMemcpyFromSymbol of the unit's __device__ array
    assert rc == 0, "%s = %d" % (name, rc)
    return out.reshape(WAVES, WORDS)


def _q(x):
    return "mean %.3f  p10 %.3f  median %.3f  p90 %.3f" % (np.mean(x), np.percentile(x, 10), np.median(x), np.percentile(x, 90))


def report(name, rec, waves, kernel):
    rec = rec[:waves]
    rec = rec[rec[:, 3] == kernel + 1]                                    # (k_miller2_pair / k_final_exp_is_one_pair write 3 and 4)
    hw = rec[:, 0] & np.uint64(0xffffffff)
    xcc = (rec[:, 0] >> np.uint64(32)) & np.uint64(0xf)
    slot, simd, cu, sh, se = hw & np.uint64(0xf), (hw >> np.uint64(4)) & np.uint64(3), (hw >> np.uint64(8)) & np.uint64(0xf), (hw >> np.uint64(12)) & np.uint64(1), (hw >> np.uint64(13)) & np.uint64(7)
    t0, t1 = rec[:, 1].astype(np.int64), rec[:, 2].astype(np.int64)
    start, span = t0.min(), t1.max() - t0.min()
    print("%s: %d waves recorded, span %d ticks = %.3f ms at 100 MHz; mean wave life %.3f of the span" % (name, len(rec), span, span / 1e5, np.mean(t1 - t0) / span))
    groups = {}
    for i in range(len(rec)):
        groups.setdefault((int(xcc[i]), int(se[i]), int(sh[i]), int(cu[i]), int(simd[i])), []).append(i)
    sizes = {}
    for g in groups.values():
        sizes[len(g)] = sizes.get(len(g), 0) + 1
    print("  SIMDs seen %d (XCCs %d); waves per SIMD: %s" % (len(groups), len(set(k[0] for k in groups)), ", ".join("%d x %d" % (v, k) for k, v in sorted(sizes.items()))))
    two = [g for g in groups.values() if len(g) == 2]
    if not two:
        print("  no SIMD held exactly two waves")
        return
    first, second, late_entry, parity, older_first, low_first = [], [], [], 0, 0, 0
    for a, b in two:
        low_first += int(t1[a if slot[a] < slot[b] else b] <= t1[b if slot[a] < slot[b] else a])
        if t0[b] < t0[a] or (t0[b] == t0[a] and slot[b] < slot[a]):
            a, b = b, a                                                    # a entered first: the older wave
        first.append((min(t1[a], t1[b]) - start) / span)
        second.append((max(t1[a], t1[b]) - start) / span)
        late_entry.append((t0[b] - start) / span)
        parity += int((int(slot[a]) ^ int(slot[b])) & 1)
        older_first += int(t1[a] <= t1[b])
    print("  SIMDs with two waves: %d" % len(two))
    print("  exit of the FIRST wave to leave, fraction of the span:   %s" % _q(first))
    print("  exit of the SECOND wave to leave, fraction of the span:  %s" % _q(second))
    print("  entry of the later-entering wave, fraction of the span:  %s" % _q(late_entry))
    print("  the wave that entered first also left first on %d of %d SIMDs" % (older_first, len(two)))
    print("  the wave with the lower slot id left first on %d of %d SIMDs" % (low_first, len(two)))
    print("  the two wave-slot ids of a SIMD differ in bit 0 on %d of %d SIMDs; slot ids seen: %s" % (parity, len(two), sorted(set(int(s) for s in slot))))


def main():
    so = os.path.abspath(sys.argv[1])
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
    import torch
    lib = C.CDLL(so)
    lib.blsmi_init(0)
    import bench
    from bls_amd import engine, _native
    _native._lib = lib
    g1, g2 = bench.synth_inputs(engine, n, 0)
    dev = torch.device("cuda", 0)
    a, b = torch.from_numpy(g1).to(dev), torch.from_numpy(g2).to(dev)
    o = torch.zeros((n, 72), dtype=torch.int64, device=dev)
    for _ in range(2):                                                     # the second call's records stay
        rc = lib.blsmi_pairing_batch_dev(C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), C.c_void_p(o.data_ptr()), C.c_size_t(n), None)
        assert rc == 0, rc
        torch.cuda.synchronize()
    waves = (n + 31) // 32
    assert waves <= WAVES, "the census arrays hold %d waves" % WAVES
    print("%s  n = %d  (%d waves a kernel)" % (os.path.basename(so), n, waves))
    report("k_miller1h_pair", read_records(lib, "blsmi_census_read_miller"), waves, 0)
    report("k_final_exp_pair", read_records(lib, "blsmi_census_read_fe"), waves, 1)


if __name__ == "__main__":
    main()
