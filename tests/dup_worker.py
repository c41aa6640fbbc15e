"""Worker of tests/test_gpu_round3.py::test_device_duplicate_table_and_its_fallback: own process so that BLSMI_DUP_FORCE_SORT (read by
the library) can differ per run.  VerifyAggregate over n > 4096 messages -- the duplicate rejection then runs on the device (k_util.hip),
or, with the environment hook, through its host fallback -- for resident and host buffers.  The duplicate, empty and all-equal sets keep the
aggregate of the original messages, so the pairing equation fails there as well; "_dup_resigned" signs the changed position again, so that
the rule alone rejects (tests/test_gpu_dup_rule.py runs a whole corpus of such cases).  Prints one JSON line."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    from bls_amd import engine as eng
    from gpu_common import P, RC, sk_bytes
    from test_gpu_round3 import _aggregate_case, _dev
    eng.init(0)
    ck = {}
    for group in ("g2pubs", "g1pubs"):
        n = 5000
        msgs, pks, agg, o = _aggregate_case(group, n, 4242)
        host = eng.g2pubs_verify_aggregate if group == "g2pubs" else eng.g1pubs_verify_aggregate

        def dev_call(ms, agg=agg):
            buf = np.frombuffer(b"".join(ms) or b"\0", dtype=np.uint8)
            off = np.zeros(len(ms) + 1, dtype=np.uint64); off[1:] = np.cumsum([len(m) for m in ms])
            d_m, d_o, d_k = _dev(buf), _dev(off), _dev(b"".join(pks))
            return eng.verify_aggregate_dev(group, d_m.data_ptr(), d_o.data_ptr(), d_k.data_ptr(), agg, len(ms))
        ck[group + "_true"] = dev_call(msgs) is True and host(msgs, b"".join(pks), agg) is True
        dup = list(msgs); dup[n - 1] = dup[7]
        ck[group + "_dup"] = dev_call(dup) is False and host(dup, b"".join(pks), agg) is False
        xs = P.XORShift(4242)                                                # (_aggregate_case's keys; position n - 1 has key (n - 1) % 8)
        sk = int.from_bytes([sk_bytes(xs) for _ in range(8)][(n - 1) % 8], "big")
        new, old = o.sign(dup[n - 1], sk.to_bytes(32, "big")), o.sign(msgs[n - 1], (P.R_ORDER - sk).to_bytes(32, "big"))   # (old: negated)
        summ = RC.g1_sum if group == "g2pubs" else RC.g2_sum
        agg2 = summ(agg + new + old, 3)
        ck[group + "_dup_resigned"] = o.verify(dup[n - 1], pks[n - 1], new) is True and dev_call(dup, agg2) is False and host(dup, b"".join(pks), agg2) is False
        # the control: the same exchange with a message that occurs nowhere else verifies, so key and negation are in step with _aggregate_case
        near = list(msgs); near[n - 1] = dup[7] + b"\0"
        agg3 = summ(agg + o.sign(near[n - 1], sk.to_bytes(32, "big")) + old, 3)
        ck[group + "_near_dup_resigned"] = len(set(near)) == n and dev_call(near, agg3) is True and host(near, b"".join(pks), agg3) is True
        emp = list(msgs); emp[1234] = b""
        ck[group + "_empty"] = dev_call(emp) is False and host(emp, b"".join(pks), agg) is False
        many = [msgs[0]] * n                                                 # every message equal: one long run of collisions, first comparison hits
        ck[group + "_all_equal"] = dev_call(many) is False and host(many, b"".join(pks), agg) is False
    print("DUP_RESULT " + json.dumps({"forced": bool(os.environ.get("BLSMI_DUP_FORCE_SORT")), "checks": ck, "ok": all(ck.values())}), flush=True)


if __name__ == "__main__":
    main()
