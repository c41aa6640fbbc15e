"""VerifyAggregate from the host's point of view: ms per call at the sizes where the host code shows -- a 1-signer and a 128-signer aggregate of
both packages from host buffers; 2 304 and 8 192 signers from host buffers and resident; the 65 536- and 2^20-signer g2pubs aggregate
resident and from host buffers; one verify_batch_rlc call per package at 32 768; and the smallest calls, where the host's cost per launch shows
most: a lone Pairing, g2pubs Verify and g1pubs Verify at 1 and 2 304 tuples from host buffers.  One process is one run: it prints `leg median_ms` for
every leg.  To compare two builds, start it alternately with and without BLSMI_LIB (bls_amd/_native.py), several runs each.  The points
are well-formed but no signatures (tools/options_launch_trace.py's workload): the verdict is 0 at the end of the same work.  GPU box only."""
import hashlib, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
from bls_amd import engine as E
E.init(0)
dev = torch.device("cuda", 0)
nk, nmax = 256, 1 << 20
sk = b"".join(hashlib.sha256(b"time-sk-%d" % i).digest()[:31].rjust(32, b"\0") for i in range(nk))
g1k, g2k = E.g1_mul_generator_batch(sk, nk)[0], E.g2_mul_generator_batch(sk, nk)[0]
g1, g2 = np.ascontiguousarray(np.tile(g1k, (nmax // nk, 1))), np.ascontiguousarray(np.tile(g2k, (nmax // nk, 1)))
msgbuf = np.frombuffer(b"".join(hashlib.sha256(int(i).to_bytes(8, "little")).digest() for i in range(nmax)), dtype=np.uint8)


def packed(n):
    p = E.PackedMsgs([]); p.buf = msgbuf[:32 * n]; p.off = np.arange(n + 1, dtype=np.uint64) * 32; p.n = n
    return p


def put(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).to(dev)


def leg(name, fn, reps):
    fn(); fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    print("%s %.4f" % (name, 1e3 * float(np.median(ts))), flush=True)


for n, reps in ((1, 200), (128, 200), (2304, 60), (8192, 40)):
    pm = packed(n)
    leg("g2pubs.VerifyAggregate/host/%d" % n, lambda: E.g2pubs_verify_aggregate(pm, g2[:n], g1[0]), reps)
    leg("g1pubs.VerifyAggregate/host/%d" % n, lambda: E.g1pubs_verify_aggregate(pm, g1[:n], g2[0]), reps)
    if n >= 2304:
        d_m, d_o, d_2, d_1 = put(pm.buf), put(pm.off), put(g2[:n]), put(g1[:n])
        leg("g2pubs.VerifyAggregate/resident/%d" % n, lambda: E.verify_aggregate_dev("g2pubs", d_m.data_ptr(), d_o.data_ptr(), d_2.data_ptr(), g1[0], n), reps)
        leg("g1pubs.VerifyAggregate/resident/%d" % n, lambda: E.verify_aggregate_dev("g1pubs", d_m.data_ptr(), d_o.data_ptr(), d_1.data_ptr(), g2[0], n), reps)
for n, reps in ((65536, 20), (1 << 20, 7)):
    pm = packed(n)
    d_m, d_o, d_2 = put(pm.buf), put(pm.off), put(g2[:n])
    leg("g2pubs.VerifyAggregate/resident/%d" % n, lambda: E.verify_aggregate_dev("g2pubs", d_m.data_ptr(), d_o.data_ptr(), d_2.data_ptr(), g1[0], n), reps)
    leg("g2pubs.VerifyAggregate/host/%d" % n, lambda: E.g2pubs_verify_aggregate(pm, g2[:n], g1[0]), reps)
n = 32768
pm = packed(n)
one = np.ones(n, dtype=np.uint64)
leg("g2pubs.VerifyBatchRlc/host/%d" % n, lambda: E.g2pubs_verify_batch_rlc(pm, g2[:n], g1[:n], scalars=None), 7)
leg("g1pubs.VerifyBatchRlc/host/%d" % n, lambda: E.g1pubs_verify_batch_rlc(pm, g1[:n], g2[:n], scalars=None), 7)
for n, reps in ((1, 200), (2304, 60)):
    pm = packed(n)
    leg("Pairing/host/%d" % n, lambda: E.pairing_batch(g1[:n], g2[:n], n), reps)
    leg("g2pubs.Verify/host/%d" % n, lambda: E.g2pubs_verify_batch(pm, g2[:n], g1[:n]), reps)
    leg("g1pubs.Verify/host/%d" % n, lambda: E.g1pubs_verify_batch(pm, g1[:n], g2[:n]), reps)
E.shutdown()
