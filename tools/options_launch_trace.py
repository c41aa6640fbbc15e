"""Which kernels the entry points launch under each environment setting: the behavioural record of the option table (route.h) and of
the way the library reads its environment.  One fresh child process per configuration (the environment is read once, at
initialisation), one after the other, each under its own time limit; the first failure ends the run.  A child switches
blsmi_set_profiling on, makes one g2pubs Verify, one g1pubs Verify, one VerifyWithDomain, one Pairing and one g2pubs VerifyAggregate
call at each size and prints the kernel names of blsmi_last_profile in launch order.  The verdicts are not looked at (the signatures
are well-formed points, not signatures): the kernels a call runs do not depend on them.
    python tools/options_launch_trace.py > profiles/options_launch_trace.txt
Two builds of the library that route alike print the same bytes (BLSMI_LIB selects another build, bls_amd/_native.py)."""
import ctypes
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1000, 4096, 12288, 65536)
# (environment, arguments of blsmi_set_row_threshold before initialisation or None)
CONFIGS = [({}, None)] + [({k: v}, None) for k, v in (
    ("BLSMI_LAYOUT", "single"), ("BLSMI_GEN_LINES", "0"), ("BLSMI_HASH_G2_PAIR", "0"), ("BLSMI_HASH_G1_SPLIT", "0"), ("BLSMI_COFAC2_PAIR", "0"),
    ("BLSMI_LAT_MAX", "1024"), ("BLSMI_ROW_MAX", "0"), ("BLSMI_QUAD_MAX", "0"), ("BLSMI_ROW_SIDE", "0"), ("BLSMI_SIG_SIDE_MAX", "0"),
    ("BLSMI_SWU_WAVE_MAX", "0"), ("BLSMI_DUP_FORCE_SORT", "0"))] + [({"BLSMI_ROW_MAX": "8192"}, (2048, 0))]
CHILD_LIMIT_S = 240


def child(row_threshold):
    sys.path.insert(0, ROOT)
    import numpy as np
    from bls_amd import engine as E, _native
    lib = _native.load()
    if row_threshold:
        E.set_row_threshold(*row_threshold)                                # before the library initialises: the API's value must outlive it
    nk, nmax = 256, max(SIZES)
    sk = b"".join(hashlib.sha256(b"trace-sk-%d" % i).digest()[:31].rjust(32, b"\0") for i in range(nk))
    g1 = np.tile(E.g1_mul_generator_batch(sk, nk)[0], (nmax // nk, 1))
    g2 = np.tile(E.g2_mul_generator_batch(sk, nk)[0], (nmax // nk, 1))
    msgs = [b"launch trace %d" % i for i in range(nmax)]
    msgs32 = [hashlib.sha256(m).digest() for m in msgs]
    domain = bytes(range(8))
    calls = (
        ("g2pubs.Verify", lambda n: E.g2pubs_verify_batch(msgs[:n], g2[:n], g1[:n])),
        ("g1pubs.Verify", lambda n: E.g1pubs_verify_batch(msgs[:n], g1[:n], g2[:n])),
        ("g1pubs.VerifyWithDomain", lambda n: E.g1pubs_verify_with_domain_batch(msgs32[:n], domain, g1[:n], g2[:n])),
        ("Pairing", lambda n: E.pairing_batch(g1[:n], g2[:n], n)),
        ("g2pubs.VerifyAggregate", lambda n: E.g2pubs_verify_aggregate(msgs[:n], g2[:n], g1[0])),
    )
    buf = ctypes.create_string_buffer(1 << 16)
    lib.blsmi_set_profiling(1)
    lib.blsmi_last_profile(buf, ctypes.c_size_t(len(buf)))                 # forget the set-up's kernels
    for name, call in calls:
        for n in SIZES:
            call(n)
            lib.blsmi_last_profile(buf, ctypes.c_size_t(len(buf)))
            print("%s %d: %s" % (name, n, " ".join(item.split("=")[0] for item in buf.value.decode().split(";") if item)), flush=True)
    E.shutdown()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(tuple(int(x) for x in sys.argv[2:]))
    for env, row_threshold in CONFIGS:
        title = " ".join("%s=%s" % kv for kv in env.items()) or "defaults"
        if row_threshold:
            title += " after blsmi_set_row_threshold(%d, %d)" % row_threshold
        print("## " + title, flush=True)
        cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [str(x) for x in row_threshold or ()]
        clean = {k: v for k, v in os.environ.items() if not k.startswith("BLSMI_") or k == "BLSMI_LIB"}
        rc = subprocess.run(cmd, env=dict(clean, **env), timeout=CHILD_LIMIT_S).returncode
        if rc:
            sys.exit("options_launch_trace: `%s` ended with status %d; stopping" % (title, rc))


if __name__ == "__main__":
    main()
