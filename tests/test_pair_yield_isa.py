"""CPU (hipcc cross-compiles): where the wave-priority yield of the lane-pair pairing kernels sits in the GENERATED code
(pair_kernels.inc: BLSMI_PAIR_YIELD; compiled the way tests/test_isa_guards.py compiles the units).

s_setprio is a scalar instruction that ignores EXEC, so what matters is where the compiler left it: `s_setprio 1` before the kernel's first
call into an out-of-line core, at least one `s_setprio 0` after it.  -DBLSMI_PAIR_YIELD=0 takes every one of them out again (the A/B build),
and the lane-quad and lane-row units -- one wave per SIMD, no yield -- compile to the same priorities either way."""
import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bls_amd", "csrc")
YIELD_KERNELS = {"k_pairing_pair.hip": ["k_miller1h_pair", "k_miller1_pair", "k_miller2_pair"],
                 "k_fe_pair.hip": ["k_final_exp_pair", "k_final_exp_is_one_pair"]}
NO_YIELD_KERNELS = {"k_pairing_pair.hip": ["k_miller1x2_pair", "k_debug_pairl"], "k_fe_pair.hip": ["k_debug_final_exp_pair"]}
OTHER_UNITS = ["k_pairing_quad.hip", "k_pairing_row.hip"]
PRIO = re.compile(r"^\s+s_setprio\s+(\d+)", re.M)
CALL = re.compile(r"^\s+s_swappc_b64\b", re.M)


def _compile(unit, out, extra):
    sys.path.insert(0, ROOT)
    from bls_amd import _native
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc] + [f for f in _native._FLAGS if f != "-fPIC"] + _native._unit_flags(unit) + extra + ["-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, unit)],
                          stderr=subprocess.DEVNULL)
    return open(out).read()


def _kernel(asm, name):
    """the instructions of one kernel: from its label to the end of the function"""
    m = re.search(r"^_Z%d%s\w*:\s*(?:;.*)?$" % (len(name), name), asm, re.M)
    assert m, "no kernel %s in the unit" % name
    return asm[m.end():asm.index(".Lfunc_end", m.end())]


@pytest.fixture(scope="module")
def asms(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("pair_yield_isa")
    jobs = [(u, on) for u in list(YIELD_KERNELS) + OTHER_UNITS for on in (True, False)]
    with ThreadPoolExecutor(8) as ex:
        texts = list(ex.map(lambda j: _compile(j[0], str(d / ("%s.%d.s" % (j[0], j[1]))), [] if j[1] else ["-DBLSMI_PAIR_YIELD=0"]), jobs))
    return dict(zip(jobs, texts))


def test_yield_kernels_raise_before_the_first_core_call_and_drop_after_it(asms):
    for unit, names in YIELD_KERNELS.items():
        for name in names:
            body = _kernel(asms[(unit, True)], name)
            first_call = CALL.search(body)
            assert first_call, "%s calls no out-of-line core" % name
            prios = [(m.start(), int(m.group(1))) for m in PRIO.finditer(body)]
            assert prios and {p for _, p in prios} == {0, 1}, "%s: levels 1 and 0 only, got %s" % (name, prios)
            assert prios[0][1] == 1 and prios[0][0] < first_call.start(), "%s: s_setprio 1 comes before the first core call" % name
            assert [p for at, p in prios if p == 1] == [1], "%s raises its priority once" % name
            assert any(p == 0 and at > first_call.start() for at, p in prios), "%s: no s_setprio 0 after the first core call" % name


def test_switch_off_removes_every_priority_instruction(asms):
    for unit, names in YIELD_KERNELS.items():
        for name in names:
            assert not PRIO.search(_kernel(asms[(unit, False)], name)), "%s keeps an s_setprio with -DBLSMI_PAIR_YIELD=0" % name
        assert not PRIO.search(asms[(unit, False)]), unit


def test_kernels_outside_the_yield_have_none(asms):
    for unit, names in NO_YIELD_KERNELS.items():
        for name in names:
            assert not PRIO.search(_kernel(asms[(unit, True)], name)), name
    # every s_setprio of a lane-pair unit sits inside one of the kernels that yield: none in a shared out-of-line function
    for unit, names in YIELD_KERNELS.items():
        inside = sum(len(PRIO.findall(_kernel(asms[(unit, True)], name))) for name in names)
        assert inside == len(PRIO.findall(asms[(unit, True)])), unit


def test_quad_and_row_units_compile_to_the_same_priorities_either_way(asms):
    for unit in OTHER_UNITS:
        on, off = PRIO.findall(asms[(unit, True)]), PRIO.findall(asms[(unit, False)])
        assert on == off, unit
        assert set(on) <= {"2"}, "%s: only the hash kernels' priority 2 (fp.cuh: hash_prio)" % unit
    assert not PRIO.findall(asms[("k_pairing_quad.hip", True)])
