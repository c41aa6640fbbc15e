"""Which kernels every VerifyAggregate form launches, call by call: the behavioural record of the host code behind them (verify_host.inc:
verify_aggregate_on_ctx, aggregate_shard_dev, aggregate_tail).  One fresh child process under a time limit switches blsmi_set_profiling
on and, per call, prints the kernel names of blsmi_last_profile in launch order -- the call's main stream; the side streams' launches
(sig_side_start) are not logged -- and then the verdict.  The calls: every form at n = 0, 1, 65, 2 304, 8 192, 16 384 and 65 536 (the
wave, row, quad and pair routes; 65 536 takes the g2pubs cofactor-power route), distinct messages and one repeated message, with
"dup_force_sort" off and on; aggregate_partial at 65 and 65 536; one verify_batch_rlc call per package at n = 65 (sig_side_start_dev,
aggregate_tail).  The workload is tools/options_launch_trace.py's: 256 generated keys tiled, well-formed points that are no signatures, so
every verdict but the empty calls' is 0 -- the kernels a call runs do not depend on that.
    python tools/aggregate_launch_trace.py > profiles/r12_aggregate_host_trace.txt
Two builds of the library that launch alike print the same bytes (BLSMI_LIB selects another build, bls_amd/_native.py)."""
import ctypes
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (0, 1, 65, 2304, 8192, 16384, 65536)
CHILD_LIMIT_S = 420


def child():
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from bls_amd import engine as E, _native
    lib = _native.load()
    dev = torch.device("cuda", 0)
    nk, nmax = 256, max(SIZES)
    sk = b"".join(hashlib.sha256(b"trace-sk-%d" % i).digest()[:31].rjust(32, b"\0") for i in range(nk))
    g1 = np.tile(E.g1_mul_generator_batch(sk, nk)[0], (nmax // nk, 1))
    g2 = np.tile(E.g2_mul_generator_batch(sk, nk)[0], (nmax // nk, 1))
    j1 = np.tile(E.g1_mul_generator_batch_jac(sk, nk), (nmax // nk, 1))
    j2 = np.tile(E.g2_mul_generator_batch_jac(sk, nk), (nmax // nk, 1))
    msgs = [b"launch trace %d" % i for i in range(nmax)]
    msgs32 = [hashlib.sha256(m).digest() for m in msgs]
    domain = bytes(range(8))
    tables = E.PreparedKeys(g2[:nk].tobytes(), nk)                         # with key_idx: tuple t reads table t mod 256
    own = E.PreparedKeys(g2.tobytes(), nmax)                               # without: tuple t reads table t
    buf = ctypes.create_string_buffer(1 << 16)

    def put(a):
        a = np.ascontiguousarray(a)
        if a.dtype in (np.uint64, np.uint32):
            a = a.view(np.int64 if a.dtype == np.uint64 else np.int32)
        return torch.from_numpy(a.copy() if a.size else np.zeros(1, a.dtype)).to(dev)

    def show(name, call):
        lib.blsmi_last_profile(buf, ctypes.c_size_t(len(buf)))             # forget what lies between the calls
        verdict = call()
        lib.blsmi_last_profile(buf, ctypes.c_size_t(len(buf)))
        names = " ".join(item.split("=")[0] for item in buf.value.decode().split(";") if item)
        print("%s: %s -> %s" % (name, names, verdict), flush=True)

    def forms(n, ms, ms32, tag):
        """every form over the first n tuples; ms / ms32: their messages (ragged / 32 bytes)"""
        packed = E.PackedMsgs(ms)
        idx = (np.arange(n, dtype=np.uint32) % nk)
        d_m, d_o, d_m32, d_dom = put(packed.buf), put(packed.off), put(np.frombuffer(b"".join(ms32) or b"\0", np.uint8)), put(np.frombuffer(domain, np.uint8))
        d_g1, d_g2, d_idx = put(g1[:n]), put(g2[:n]), put(idx)
        p = lambda t: t.data_ptr()
        for name, call in (
            ("g2pubs.VerifyAggregate", lambda: E.g2pubs_verify_aggregate(packed, g2[:n], g1[0])),
            ("g2pubs.VerifyAggregate_jac", lambda: E.g2pubs_verify_aggregate_jac(packed, j2[:n], j1[0])),
            ("g2pubs.VerifyAggregate_dev", lambda: E.verify_aggregate_dev("g2pubs", p(d_m), p(d_o), p(d_g2), g1[0], n)),
            ("g2pubs.VerifyAggregate_prepared[idx]", lambda: E.g2pubs_verify_aggregate_prepared(packed, tables, idx, g1[0])),
            ("g2pubs.VerifyAggregate_prepared", lambda: E.g2pubs_verify_aggregate_prepared(packed, own, None, g1[0])),
            ("g2pubs.VerifyAggregate_prepared_jac[idx]", lambda: E.g2pubs_verify_aggregate_prepared_jac(packed, tables, idx, j1[0])),
            ("g2pubs.VerifyAggregate_prepared_jac", lambda: E.g2pubs_verify_aggregate_prepared_jac(packed, own, None, j1[0])),
            ("g2pubs.VerifyAggregate_prepared_dev[idx]", lambda: E.g2pubs_verify_aggregate_prepared_dev(p(d_m), p(d_o), tables.ptr, p(d_idx) if n else 0, g1[0], n)),
            ("g2pubs.VerifyAggregate_prepared_dev", lambda: E.g2pubs_verify_aggregate_prepared_dev(p(d_m), p(d_o), own.ptr, 0, g1[0], n)),
            ("g1pubs.VerifyAggregate", lambda: E.g1pubs_verify_aggregate(packed, g1[:n], g2[0])),
            ("g1pubs.VerifyAggregate_jac", lambda: E.g1pubs_verify_aggregate_jac(packed, j1[:n], j2[0])),
            ("g1pubs.VerifyAggregate_dev", lambda: E.verify_aggregate_dev("g1pubs", p(d_m), p(d_o), p(d_g1), g2[0], n)),
            ("g1pubs.VerifyAggregateWithDomain", lambda: E.g1pubs_verify_aggregate_with_domain(ms32, domain, g1[:n], g2[0])),
            ("g1pubs.VerifyAggregateWithDomain_jac", lambda: E.g1pubs_verify_aggregate_with_domain_jac(ms32, domain, j1[:n], j2[0])),
            ("g1pubs.VerifyAggregateWithDomain_dev", lambda: E.verify_aggregate_with_domain_dev(p(d_m32), p(d_dom), p(d_g1), g2[0], n)),
        ):
            show("%s %d %s" % (name, n, tag), call)

    lib.blsmi_set_profiling(1)
    for force in (0, 1):
        E.set_option("dup_force_sort", force)
        for n in SIZES:
            forms(n, msgs[:n], msgs32[:n], "distinct sort=%d" % force)
            if n >= 2:
                forms(n, msgs[:n - 1] + msgs[:1], msgs32[:n - 1] + msgs32[:1], "repeated sort=%d" % force)
    E.set_option("dup_force_sort", 0)
    for n in (65, 65536):
        show("g2pubs.AggregatePartial %d" % n, lambda: bool(E.aggregate_partial("g2pubs", msgs[:n], g2[:n])[1]))
        show("g1pubs.AggregatePartial %d" % n, lambda: bool(E.aggregate_partial("g1pubs", msgs[:n], g1[:n])[1]))
    n = 65
    E.set_option("rlc_min", 1)                                             # (below "rlc_min", 32 768 by default, the call would take the per-tuple path)
    one = [1] * n                                                          # the caller's scalars: the same run every time
    show("g2pubs.VerifyBatchRlc %d" % n, lambda: int(E.g2pubs_verify_batch_rlc(msgs[:n], g2[:n], g1[:n], scalars=one)[0].sum()))
    show("g1pubs.VerifyBatchRlc %d" % n, lambda: int(E.g1pubs_verify_batch_rlc(msgs[:n], g1[:n], g2[:n], scalars=one)[0].sum()))
    show("g1pubs.VerifyWithDomainBatchRlc %d" % n, lambda: int(E.g1pubs_verify_with_domain_batch_rlc(msgs32[:n], domain, g1[:n], g2[:n], scalars=one)[0].sum()))
    own.close(); tables.close()
    E.shutdown()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child()
    clean = {k: v for k, v in os.environ.items() if not k.startswith("BLSMI_") or k == "BLSMI_LIB"}
    rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=clean, timeout=CHILD_LIMIT_S).returncode
    if rc:
        sys.exit("aggregate_launch_trace: the child ended with status %d" % rc)


if __name__ == "__main__":
    main()
