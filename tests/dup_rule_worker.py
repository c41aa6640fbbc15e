"""Worker of tests/test_gpu_dup_rule.py::test_split_call_host_thread_beside_the_shards: own process, because the split of the library
(BLSMI_SHARDS logical shards) and BLSMI_DUP_FORCE_SORT are read when the library initialises.  A split VerifyAggregate screens for
duplicates on a host thread beside the shards; here the rule alone decides every verdict (dup_cases.py: the aggregate is a correct
signature of the messages as they stand).  argv[1]: a pickle of plain data from the parent, which signed and checked the premise --
{group: {"keys": bytes, "msgs": [bytes], "agg": bytes, "cases": [{"name", "changes": {position: message}, "agg", "model"}]}} -- so the
worker needs no oracle and computes nothing but the library's verdicts.  Prints one JSON line."""
import json
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from bls_amd import engine as eng
    with open(sys.argv[1], "rb") as fh:
        sets = pickle.load(fh)
    eng.init_devices(1)
    shards = eng.shard_count()
    out = {"devices": eng.device_count(), "shards": shards, "forced": bool(os.environ.get("BLSMI_DUP_FORCE_SORT")), "runs": {}}
    for group, s in sets.items():
        n = len(s["msgs"])
        per = (-(-n // shards) + 63) // 64 * 64                            # plan_shards(n, 64): tuples per shard
        host = eng.g2pubs_verify_aggregate if group == "g2pubs" else eng.g1pubs_verify_aggregate
        rows = []
        for c in s["cases"]:
            msgs = list(s["msgs"])
            for p, m in c["changes"].items():
                msgs[p] = m
            rows.append({"name": c["name"], "model": c["model"], "got": host(msgs, s["keys"], c["agg"]),
                         "restored": host(s["msgs"], s["keys"], s["agg"]), "shards_of_changed": sorted(p // per for p in c["changes"])})
        out["runs"][group] = rows
    eng.shutdown()
    print("DUP_RULE_RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
