"""The group operations from the host's point of view: ms per call at the sizes where the host code shows (tools/aggregate_forms_bench.py does the
same for VerifyAggregate).  For G1 and G2, from host buffers: mul_batch at 1 and 4 096 points, mul_generator_batch at 1, sum at 2 and 4 096,
sum_jac at 4 096, msm at 67 and 2^17 (the bucket method), sum_segmented over 4 096 points in 64 segments; for both packages
VerifyAggregateCommon at 128 signers and verify_batch_rlc at 32 768.  One process is one run: it prints `leg median_ms` for every leg.  To
compare two builds, start it alternately with and without BLSMI_LIB (bls_amd/_native.py), several runs each.  The points are well-formed but no
signatures (tools/options_launch_trace.py's workload): the verdict is 0 at the end of the same work.  GPU box only."""
import hashlib, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np
from bls_amd import engine as E
from gpu_common import g1_to_jac, g2_to_jac
E.init(0)
nk, nmax = 256, 1 << 17
sk = b"".join(hashlib.sha256(b"time-sk-%d" % i).digest()[:31].rjust(32, b"\0") for i in range(nk))
keys = {1: E.g1_mul_generator_batch(sk, nk)[0], 2: E.g2_mul_generator_batch(sk, nk)[0]}
pts = {g: np.ascontiguousarray(np.tile(keys[g], (nmax // nk, 1))) for g in (1, 2)}
ks = np.frombuffer(b"".join(hashlib.sha256(int(i).to_bytes(8, "little")).digest()[:31].rjust(32, b"\0") for i in range(nmax)), dtype=np.uint8).reshape(nmax, 32)
msgbuf = np.frombuffer(b"".join(hashlib.sha256(int(i).to_bytes(8, "little")).digest() for i in range(32768)), dtype=np.uint8)
to_jac = {1: g1_to_jac, 2: g2_to_jac}
jac = {g: np.ascontiguousarray(np.tile(np.frombuffer(b"".join(to_jac[g](bytes(w)) for w in keys[g]), dtype=np.uint8), 4096 // nk)) for g in (1, 2)}
seg = E.seg_offsets([64] * 64)


def packed(n):
    p = E.PackedMsgs([]); p.buf = msgbuf[:32 * n]; p.off = np.arange(n + 1, dtype=np.uint64) * 32; p.n = n
    return p


def leg(name, fn, reps):
    fn(); fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    print("%s %.4f" % (name, 1e3 * float(np.median(ts))), flush=True)


FN = {1: (E.g1_mul_batch, E.g1_mul_generator_batch, E.g1_sum, E.g1_sum_jac, E.g1_msm, E.g1_sum_segmented),
      2: (E.g2_mul_batch, E.g2_mul_generator_batch, E.g2_sum, E.g2_sum_jac, E.g2_msm, E.g2_sum_segmented)}
for g in (1, 2):
    mul, gen, add, add_jac, msm, segsum = FN[g]
    p = pts[g]
    for n, reps in ((1, 200), (4096, 40)):
        leg("g%d.mul_batch/%d" % (g, n), lambda: mul(p[:n], ks[:n], n), reps)
    leg("g%d.mul_generator_batch/1" % g, lambda: gen(ks[:1], 1), 200)
    for n, reps in ((2, 200), (4096, 60)):
        leg("g%d.sum/%d" % (g, n), lambda: add(p[:n], n), reps)
    leg("g%d.sum_jac/4096" % g, lambda: add_jac(jac[g], 4096), 60)
    for n, reps in ((67, 100), (1 << 17, 7)):
        leg("g%d.msm/%d" % (g, n), lambda: msm(p[:n], ks[:n], n), reps)
    leg("g%d.sum_segmented/4096x64" % g, lambda: segsum(p[:4096], 4096, None, seg), 60)
msg = b"group ops bench"
leg("g2pubs.VerifyAggregateCommon/host/128", lambda: E.g2pubs_verify_aggregate_common(msg, pts[2][:128], pts[1][0], 128), 200)
leg("g1pubs.VerifyAggregateCommon/host/128", lambda: E.g1pubs_verify_aggregate_common(msg, pts[1][:128], pts[2][0], 128), 200)
n = 32768
pm = packed(n)
leg("g2pubs.VerifyBatchRlc/host/%d" % n, lambda: E.g2pubs_verify_batch_rlc(pm, pts[2][:n], pts[1][:n], scalars=None), 7)
leg("g1pubs.VerifyBatchRlc/host/%d" % n, lambda: E.g1pubs_verify_batch_rlc(pm, pts[1][:n], pts[2][:n], scalars=None), 7)
E.shutdown()
