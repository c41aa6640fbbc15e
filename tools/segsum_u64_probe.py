#!/usr/bin/env python3
"""Pass 1 of the weighted G2 segmented sum, one lane per ladder (k_g2_segsum_chunk_u64) against a lane pair per ladder
(k_g2_segsum_chunk_u64_pair), kernel time from a kernel trace.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/segsum_u64_probe.py run
    python tools/segsum_u64_probe.py summarize DIR [--log profiles/r16_segsum_u64_pair.log]

`run`: for n in 1 024 and 4 096 points (16 segments of n / 16, random 64-bit scalars), blsmi_g2_sum_segmented_u64 and then
blsmi_debug_g2_sum_segmented_u64_pair, one warm-up call and three measured ones each; the two results are compared byte for byte.
`summarize`: per kernel and size the median of the three measured dispatches and their spread (max - min), in microseconds.

The criterion, fixed before the first measurement: the lane-pair kernel is the driver's default if at BOTH sizes its median
is below the one-lane kernel's by more than the spread (the larger of the two kernels' spreads at that size)."""
import csv
import glob
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = (1024, 4096)
REPS = 3
KERNELS = ("k_g2_segsum_chunk_u64", "k_g2_segsum_chunk_u64_pair")


def run():
    import numpy as np
    from bls_amd import engine
    engine.init(0)
    rng = np.random.default_rng(16)
    for n in SIZES:
        sk = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        sk[:, 0] &= 0x3f
        pts, _ = engine.g2_mul_generator_batch(sk.reshape(-1).tobytes(), n)
        pts = pts.reshape(-1).tobytes()
        r = [int(x) | 1 for x in rng.integers(0, 1 << 63, size=n, dtype=np.uint64)]
        off = engine.seg_offsets([n // 16] * 16)
        outs = []
        for fn in (engine.g2_sum_segmented_u64, engine.debug_g2_sum_segmented_u64_pair):
            for _ in range(1 + REPS):
                out, inf = fn(pts, n, r, None, off)
            outs.append(out)
        assert outs[0] == outs[1], "the two kernels disagree at n = %d" % n
        print("n = %d: 16 sums, both forms agree" % n, flush=True)


def summarize(d, log=None):
    rows = []
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            hit = re.search(r"k_g2_segsum_chunk_u64(_pair)?(?![a-z_0-9])", row["Kernel_Name"])   # (the name as the trace has it: mangled or not)
            if hit:
                rows.append((int(row["Start_Timestamp"]), hit.group(0), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
    rows.sort()
    lines = ["# pass 1 of blsmi_g2_sum_segmented_u64, kernel time from rocprofv3 --kernel-trace; median of %d after one warm-up, spread = max - min; us" % REPS,
             "%-8s %-30s %10s %10s   %s" % ("points", "kernel", "median_us", "spread_us", "runs")]
    stats = {}
    for k in KERNELS:
        mine = [t for _, name, t in rows if name == k]
        assert len(mine) == len(SIZES) * (1 + REPS), (k, len(mine))
        for i, n in enumerate(SIZES):
            stats[(n, k)] = mine[i * (1 + REPS) + 1:(i + 1) * (1 + REPS)]    # (the first of each size is the warm-up)
    keep = True
    for n in SIZES:
        med, spread = {}, {}
        for k in KERNELS:
            runs = stats[(n, k)]
            med[k], spread[k] = statistics.median(runs), max(runs) - min(runs)
            lines.append("%-8d %-30s %10.1f %10.1f   %s" % (n, k, med[k], spread[k], " ".join("%.1f" % t for t in runs)))
        faster = med[KERNELS[0]] - med[KERNELS[1]] > max(spread.values())
        keep = keep and faster
        lines.append("%-8d one lane / lane pair = %.2fx; faster by more than the spread: %s" % (n, med[KERNELS[0]] / med[KERNELS[1]], "yes" if faster else "NO"))
    lines.append("criterion (faster by more than the spread at both sizes): %s" % ("the lane-pair kernel stays" if keep else "NOT met"))
    print("\n".join(lines))
    if log:
        open(log, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "summarize":
        summarize(sys.argv[2], sys.argv[4] if len(sys.argv) >= 5 and sys.argv[3] == "--log" else None)
    else:
        run()
