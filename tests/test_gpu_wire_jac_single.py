"""-m gpu: G2 compression of in-memory points (blsmi 0.15) under BLSMI_LAYOUT=single -- a start-up switch, so the G2 compression corpus of
tests/test_gpu_wire_jac.py runs in ONE fresh child process (this file is its own worker), where every output is checked against the oracle
and the two-call route, and the profile name is asserted: the one-lane kernel k_g2_compress_jac.  The lane-pair form that
was measured beside it was dropped, so the same kernel serves the default layout; the parent compares the bytes."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":                                                   # the child process: python tests/<this file>
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

CHILD_LIMIT_S = 120


def test_g2_one_lane_compression_under_layout_single():
    from bls_amd import engine
    from test_gpu_wire_jac import compression_results
    engine.init(0)
    mine, names = compression_results(engine, 2)
    assert names == ["k_g2_compress_jac"], names
    env = dict(os.environ, BLSMI_LAYOUT="single")
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    child = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=CHILD_LIMIT_S)   # a new process, never exec
    assert child.returncode == 0, (child.returncode, child.stderr[-2000:])
    theirs = json.loads(child.stdout.strip().splitlines()[-1])
    assert theirs["names"] == ["k_g2_compress_jac"], theirs["names"]
    assert theirs["bytes"] == mine


if __name__ == "__main__":
    from bls_amd import engine
    from test_gpu_wire_jac import compression_results
    engine.init(0)
    out, names = compression_results(engine, 2, resident=False)              # (asserts every output against the oracle and the two-call route)
    print(json.dumps({"bytes": out, "names": names}))
