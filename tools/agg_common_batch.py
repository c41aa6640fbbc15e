#!/usr/bin/env python3
"""Committees in one call (blsmi 0.9) against the single-call loop, resident keys, g1pubs WithDomain.
For every shape (m committees x committee size, indices drawn from one 2^20-key G1 registry on the device):
  seq   -- m sequential blsmi_g1pubs_verify_aggregate_common_with_domain_dev calls, each over its committee's keys gathered contiguously
  batch -- one blsmi_g1pubs_verify_aggregate_common_with_domain_batch_dev call over the registry and the index array
Interleaved (seq, batch, seq, batch, ...) after a warm-up, best of --reps; the verdicts of both are checked (all 1 but one corrupted item).
usage: tools/agg_common_batch.py [--reps 5] [--shapes 1x128,16x128,...] [--log profiles/r07_agg_common_batch.log]"""
import argparse
import hashlib
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bls_amd import engine  # noqa: E402

R_ORDER = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
DOM = b"\x07\x00\x00\x00\x01\x00\x00\x00"
SHAPES = "1x128,16x128,128x128,128x512,64x2048,1x131072"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    engine.init(0)
    n = 1 << 20
    rng = np.random.default_rng(7)
    sk = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    sk[:, 0] &= 0x3f
    keys, _ = engine.g1_mul_generator_batch(sk.reshape(-1).tobytes(), n)
    d_reg = torch.from_numpy(keys.reshape(-1).copy()).to(dev)
    ski = [int.from_bytes(sk[i].tobytes(), "big") for i in range(n)]
    lines = ["# %s; registry 2^20 G1 keys on the device; best of %d, interleaved after one warm-up; ms per call" % (engine.version(), a.reps),
             "%-12s %10s %10s %8s %s" % ("shape", "seq_ms", "batch_ms", "ratio", "verdicts")]
    print(lines[0]); print(lines[1])
    for sh in a.shapes.split(","):
        m, L = (int(x) for x in sh.split("x"))
        comm = [rng.integers(0, n, size=L).astype(np.uint32) for _ in range(m)]
        msgs = [hashlib.sha256(b"%s slot %d" % (sh.encode(), j)).digest() for j in range(m)]
        ssum = b"".join((sum(ski[i] for i in c) % R_ORDER).to_bytes(32, "big") for c in comm)
        sigs, _ = engine.g1pubs_sign_with_domain_batch(msgs, DOM, ssum)
        sigs = sigs.copy()
        bad = m // 2
        sigs[bad] = sigs[(bad + 1) % m] if m > 1 else np.zeros(192, np.uint8)
        idx = np.concatenate(comm)
        off = engine.seg_offsets([L] * m)
        d_idx = torch.from_numpy(idx).to(dev)
        d_off = torch.from_numpy(off.view(np.uint8).copy()).to(dev)
        d_sig = torch.from_numpy(sigs.reshape(-1).copy()).to(dev)
        d_msg = torch.from_numpy(np.frombuffer(b"".join(msgs), np.uint8).copy()).to(dev)
        d_dom = torch.from_numpy(np.frombuffer(DOM, np.uint8).copy()).to(dev)
        d_ok = torch.zeros(m, dtype=torch.uint8, device=dev)
        gathered = [d_reg.view(n, 96)[torch.from_numpy(c.astype(np.int64)).to(dev)].contiguous() for c in comm]
        torch.cuda.synchronize()

        def seq():
            return [engine.verify_aggregate_common_dev("g1pubs", gathered[j].data_ptr(), L, msgs[j], bytes(sigs[j]), domain=DOM) for j in range(m)]

        def batch():
            engine.verify_aggregate_common_batch_dev("g1pubs", d_msg.data_ptr(), d_dom.data_ptr(), d_reg.data_ptr(), n, d_idx.data_ptr(), d_off.data_ptr(),
                                                     d_sig.data_ptr(), d_ok.data_ptr(), m, domain=True)
            return [bool(x) for x in d_ok.cpu().numpy()]

        want = [j != bad for j in range(m)]
        vs, vb = seq(), batch()
        ok = vs == want and vb == want
        ts, tb = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter(); seq(); ts.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); batch(); tb.append(time.perf_counter() - t0)
        s_ms, b_ms = 1e3 * min(ts), 1e3 * min(tb)
        line = "%-12s %10.2f %10.2f %8.1f %s" % (sh, s_ms, b_ms, s_ms / b_ms, "ok" if ok else "MISMATCH")
        print(line, flush=True)
        lines.append(line)
    if a.log:
        open(a.log, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
