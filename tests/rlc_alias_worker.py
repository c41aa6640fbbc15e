"""Worker of tests/test_gpu_rlc.py::test_split_call_per_shard: own process, because the device list is fixed when the library initialises.
BLSMI_DEVICE_ALIAS=0,0 and a small BLSMI_SHARD_MIN split a randomised batch verification over two logical devices; each shard runs its own
combined check.  Prints "RLC_ALIAS ok" or what went wrong."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    from bls_amd import engine as eng
    eng.init_devices(0)
    assert eng.device_count() == 2 and eng.shard_count() == 2, (eng.device_count(), eng.shard_count())
    n = 512
    sks = b"".join(hashlib.sha256(b"alias-rlc-%d" % i).digest()[:31].rjust(32, b"\0") for i in range(n))
    msgs = [b"split %d" % i for i in range(n)]
    pks, _ = eng.g2_mul_generator_batch(sks, n)
    sigs, _ = eng.g2pubs_sign_batch(msgs, sks)
    p, s = np.asarray(pks, np.uint8).tobytes(), np.asarray(sigs, np.uint8).tobytes()
    ok, bm, comb = eng.g2pubs_verify_batch_rlc(msgs, p, s)
    problems = []
    if comb != 1 or not ok.all():
        problems.append(("clean", comb, int(ok.sum())))
    m = list(msgs); m[400] = b"forged"                                          # the second shard only
    ok, bm, comb = eng.g2pubs_verify_batch_rlc(m, p, s)
    want = np.ones(n, bool); want[400] = False
    if comb != 0 or not np.array_equal(ok, want) or not np.array_equal(bm, np.packbits(want.astype(np.uint8), bitorder="little")):
        problems.append(("one shard corrupted", comb, np.flatnonzero(~ok).tolist()))
    vok, vbm = eng.g2pubs_verify_batch(m, p, s)
    if not np.array_equal(vbm, bm):
        problems.append("bitmap differs from verify_batch")
    print("RLC_ALIAS " + ("ok" if not problems else repr(problems)))


if __name__ == "__main__":
    main()
