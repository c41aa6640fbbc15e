#!/usr/bin/env python3
"""Many committee aggregates in one call: the randomised form (blsmi 0.16) against the per-item form (blsmi 0.9), resident keys.
g1pubs WithDomain and g2pubs, one 2^20-key registry of each group on the device.  For every shape m x L x d (m committees of L indices
drawn from the registry, d distinct messages, item j under message j mod d):
  batch -- one blsmi_g?pubs_verify_aggregate_common*_batch_dev call (the m messages expanded)
  rlc   -- one blsmi_g?pubs_verify_aggregate_common*_batch_rlc_dev call (the table of d messages and msg_idx), scalars drawn by the library
Interleaved (batch, rlc, batch, rlc, ...) after one warm-up of each; the median of --reps with the spread (min .. max); all items valid,
and with one bad item (a neighbour's signature).  The verdicts of both calls and `combined` are checked.
usage: tools/agg_common_rlc.py [--reps 5] [--shapes 128x128x128,...] [--log profiles/r16_agg_common_rlc.log]"""
import argparse
import hashlib
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bls_amd import engine  # noqa: E402

R_ORDER = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
DOM = b"\x07\x00\x00\x00\x01\x00\x00\x00"
SHAPES = "128x128x128,1024x128x64,1024x512x64,4096x128x64,4096x128x4096"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    engine.init(0)
    n = 1 << 20
    rng = np.random.default_rng(16)
    sk = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    sk[:, 0] &= 0x3f
    ski = np.array([int.from_bytes(sk[i].tobytes(), "big") for i in range(n)], dtype=object)

    def t(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)
    lines = ["# %s; registry 2^20 keys on the device; median of %d (min .. max), interleaved after one warm-up; ms per call" % (engine.version(), a.reps),
             "%-10s %-18s %-6s %24s %24s %7s  %s" % ("kind", "m x L x d", "items", "batch_ms (0.9)", "rlc_ms (0.16)", "ratio", "verdicts")]
    print("\n".join(lines), flush=True)
    for kind in ("g1pubs_wd", "g2pubs"):
        group = "g2pubs" if kind == "g2pubs" else "g1pubs"
        keys, _ = (engine.g2_mul_generator_batch if kind == "g2pubs" else engine.g1_mul_generator_batch)(sk.reshape(-1).tobytes(), n)
        d_reg = t(keys)
        del keys
        for sh in a.shapes.split(","):
            m, L, d = (int(x) for x in sh.split("x"))
            comm = [rng.integers(0, n, size=L).astype(np.uint32) for _ in range(m)]
            table = [hashlib.sha256(b"%s message %d" % (sh.encode(), g)).digest() for g in range(d)]
            mi = np.arange(m, dtype=np.uint32) % d
            msgs = [table[g] for g in mi]
            ssum = b"".join((int(ski[c].sum()) % R_ORDER).to_bytes(32, "big") for c in comm)
            if kind == "g2pubs":
                sigs, _ = engine.g2pubs_sign_batch(msgs, ssum)
                moff = lambda k: t(np.arange(k + 1, dtype=np.uint64) * 32)   # noqa: E731  (32-byte messages: offsets 0, 32, ...)
                d_tab_off, d_msg_off = moff(d), moff(m)
            else:
                sigs, _ = engine.g1pubs_sign_with_domain_batch(msgs, DOM, ssum)
                d_tab_off = d_msg_off = t(np.frombuffer(DOM, np.uint8))
            sigs = np.asarray(sigs, np.uint8).reshape(m, -1).copy()
            d_idx, d_off, d_mi = t(np.concatenate(comm)), t(engine.seg_offsets([L] * m)), t(mi)
            d_tab, d_msg = t(np.frombuffer(b"".join(table), np.uint8)), t(np.frombuffer(b"".join(msgs), np.uint8))
            d_ok = torch.zeros(m, dtype=torch.uint8, device=dev)
            for case in ("valid", "one bad"):
                s = sigs.copy()
                bad = m // 2
                if case == "one bad":
                    s[bad] = sigs[(bad + 1) % m]
                d_sig = t(s)
                want = [case == "valid" or j != bad for j in range(m)]
                torch.cuda.synchronize()

                def batch():
                    engine.verify_aggregate_common_batch_dev(group, d_msg.data_ptr(), d_msg_off.data_ptr(), d_reg.data_ptr(), n, d_idx.data_ptr(), d_off.data_ptr(),
                                                             d_sig.data_ptr(), d_ok.data_ptr(), m, domain=(kind != "g2pubs"))
                    return [bool(x) for x in d_ok.cpu().numpy()], None

                def rlc():
                    comb = engine.verify_aggregate_common_batch_rlc_dev(group, d_tab.data_ptr(), d_tab_off.data_ptr(), d, d_mi.data_ptr(), d_reg.data_ptr(), n, d_idx.data_ptr(),
                                                                        d_off.data_ptr(), d_sig.data_ptr(), d_ok.data_ptr(), m, domain=(kind != "g2pubs"))
                    return [bool(x) for x in d_ok.cpu().numpy()], comb
                vb, vr = batch(), rlc()
                ok = vb[0] == want and vr == (want, 1 if case == "valid" else 0)
                tb, tr = [], []
                for _ in range(a.reps):
                    t0 = time.perf_counter(); batch(); tb.append(1e3 * (time.perf_counter() - t0))
                    t0 = time.perf_counter(); rlc(); tr.append(1e3 * (time.perf_counter() - t0))
                fmt = lambda v: "%8.2f (%.2f .. %.2f)" % (statistics.median(v), min(v), max(v))   # noqa: E731
                line = "%-10s %-18s %-6s %24s %24s %7.2f  %s" % (kind, sh, case.split()[0], fmt(tb), fmt(tr), statistics.median(tb) / statistics.median(tr), "ok" if ok else "MISMATCH")
                print(line, flush=True)
                lines.append(line)
    if a.log:
        open(a.log, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
