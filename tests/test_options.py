"""The option table of bls_amd/csrc/route.h against what the library did before the table existed: the names blsmi_set_option knows,
every default, every environment variable and the rule it is read by (their quirks included), and the rule that a row set through the
API is not touched by its variable.  Asked through the routing driver (tests/native/route_table.cc: `options`, `env`) and, for
blsmi_set_option itself, in a child process that loads libblsmi.so (no device needed).  The expectations below were written down from
the code the table replaced, not from the table."""
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RUNTIME_NAMES = """agg_cofactor_pow msm_sort dup_force_sort lat_rolled crowd_quad row_side row_side_g2pubs hash_row_min
    hash_row_max hash_quad_min hash_quad_max hash_oct_min hash_oct_max hash_g1_quad_min hash_g1_quad_max swu_row_max combine_mid_max
    crowd_floor assume_load rlc_min segsum_chunk""".split()
# set while running through a function of their own (blsmi_set_latency_threshold, _quad_threshold, _row_threshold, _mul_assume_subgroup)
SETTER_MEMBERS = ["lat_max", "quad_max", "row_min", "row_max", "mul_subgroup"]
DEFAULTS = dict(
    lat_max=8192, quad_max=16384, quad_min=5632, row_min=2048, row_max=8192, crowd_quad=1, crowd_floor=1536, assume_load=0,
    hash_row_min=2048, hash_row_max=4096, hash_quad_min=4097, hash_quad_max=16384, hash_oct_min=2048, hash_oct_max=7168,
    hash_g1_quad_min=1280, hash_g1_quad_max=32768, swu_row_max=4096, row_side=1, row_side_g2pubs=1, agg_cofactor_pow=1, msm_sort=1,
    lat_rolled=1, dup_force_sort=0, mul_subgroup=1, pair_layout=1, use_gen_lines=1, hash_g2_pair=1, hash_g1_split=1, swu_wave_max=512,
    fixed_wave_max=2048, sig_side_max=-1, rlc_min=32768, segsum_chunk=0,
    combine_mid_max=8192, side_max=131072, msm_bucket_min=1 << 17, cofac2_pair=1, hash_g2_pair_redo_every=0)
# variable -> (member, rule).  The rules, as {value: member afterwards} with None for "unset":
NUMBER = {None: "default", "0": 0, "1024": 1024, "12abc": 12, "abc": 0}                   # strtoull, base 10
OFF_AT_0 = {None: 1, "0": 0, "00": 0, "0x": 0, "1": 1, "no": 1, "": 1}                    # off iff the first character is '0'
ATOI = {None: 1, "0": 0, "00": 0, "2": 1, "1": 1, "yes": 0, "": 0}                        # on iff atoi() is not 0
VARIABLES = {
    "BLSMI_LAT_MAX": ("lat_max", NUMBER), "BLSMI_QUAD_MAX": ("quad_max", NUMBER), "BLSMI_QUAD_MIN": ("quad_min", NUMBER),
    "BLSMI_ROW_MIN": ("row_min", NUMBER), "BLSMI_ROW_MAX": ("row_max", NUMBER), "BLSMI_CROWD_FLOOR": ("crowd_floor", NUMBER),
    "BLSMI_COMBINE_MID_MAX": ("combine_mid_max", NUMBER), "BLSMI_RLC_MIN": ("rlc_min", NUMBER), "BLSMI_SEGSUM_CHUNK": ("segsum_chunk", NUMBER),
    "BLSMI_SWU_WAVE_MAX": ("swu_wave_max", NUMBER), "BLSMI_FIXED_WAVE_MAX": ("fixed_wave_max", NUMBER), "BLSMI_SIDE_MAX": ("side_max", NUMBER),
    "BLSMI_MSM_BUCKET_MIN": ("msm_bucket_min", NUMBER), "BLSMI_HASH_G2_PAIR_REDO_EVERY": ("hash_g2_pair_redo_every", NUMBER),
    "BLSMI_AGG_COFACTOR_POW": ("agg_cofactor_pow", OFF_AT_0), "BLSMI_MSM_SORT": ("msm_sort", OFF_AT_0), "BLSMI_LAT_ROLLED": ("lat_rolled", OFF_AT_0),
    "BLSMI_CROWD_QUAD": ("crowd_quad", OFF_AT_0), "BLSMI_ROW_SIDE": ("row_side", OFF_AT_0),
    "BLSMI_HASH_G1_SPLIT": ("hash_g1_split", ATOI), "BLSMI_HASH_G2_PAIR": ("hash_g2_pair", ATOI), "BLSMI_COFAC2_PAIR": ("cofac2_pair", ATOI),
    "BLSMI_DUP_FORCE_SORT": ("dup_force_sort", {None: 0, "0": 1, "1": 1, "": 1}),          # on iff set
    "BLSMI_MUL_GENERIC": ("mul_subgroup", {None: 1, "0": 1, "1": 0, "00": 0, "": 0}),      # inverted, the whole value compared with "0"
    "BLSMI_LAYOUT": ("pair_layout", {None: 1, "single": 0, "pair": 1, "singles": 1, "": 1}),
    "BLSMI_GEN_LINES": ("use_gen_lines", {None: 1, "0": 0, "00": 1, "1": 1}),
    "BLSMI_SIG_SIDE_MAX": ("sig_side_max", {None: -1, "-1": -1, "100": 100, "0": 0, "-7": -7}),   # atoll
}
FIXED_MEMBERS = ["quad_min", "pair_layout", "use_gen_lines", "hash_g2_pair", "hash_g1_split", "hash_g2_pair_redo_every", "cofac2_pair",
                 "swu_wave_max", "fixed_wave_max", "sig_side_max", "side_max", "msm_bucket_min"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gpp = shutil.which("g++")
    if gpp is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("options") / "route_table")
    subprocess.check_call([gpp, "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "route_table.cc")])

    def run(lines):
        return subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True, check=True).stdout.splitlines()
    return run


@pytest.fixture(scope="module")
def rows(driver):
    """member -> (option name or None, variable or None, 'run-time' / 'fixed', default)"""
    out = {}
    for line in driver(["options"]):
        member, name, var, when, default = line.split()
        assert member not in out, "two rows for " + member
        out[member] = (None if name == "-" else name, None if var == "-" else var, when, int(default))
    return out


def env(driver, variables=None, explicit=()):
    """the members after apply_env over `variables`, with the rows of `explicit` marked as set through the API"""
    words = ["env"] + (["explicit=" + ",".join(explicit)] if explicit else []) + ["%s=%s" % kv for kv in (variables or {}).items()]
    (line,) = driver([" ".join(words)])
    return {k: int(v) for k, v in (kv.split("=") for kv in line.split())}


def test_run_time_names_and_defaults(rows):
    named = {m: r for m, r in rows.items() if r[0] is not None}
    assert sorted(r[0] for r in named.values()) == sorted(RUNTIME_NAMES)
    assert len(RUNTIME_NAMES) == 21
    assert all(r[2] == "run-time" for r in named.values())
    assert sorted(m for m, r in rows.items() if r[2] == "run-time" and r[0] is None) == sorted(SETTER_MEMBERS)
    assert sorted(m for m, r in rows.items() if r[2] == "fixed") == sorted(FIXED_MEMBERS)
    assert {m: r[3] for m, r in rows.items()} == DEFAULTS


def test_variables_are_the_library_s(rows):
    assert {r[1]: m for m, r in rows.items() if r[1] is not None} == {var: member for var, (member, _) in VARIABLES.items()}


def test_header_names_every_option_and_variable(rows):
    header = open(os.path.join(ROOT, "include", "blsmi.h")).read()
    words = set(re.findall(r"\w+", header))
    for member, (name, var, _, _) in rows.items():
        if name is not None:
            assert '"%s"' % name in header, name
        if var is not None:
            assert var in words, var


def test_no_environment_is_the_defaults(driver):
    assert env(driver) == DEFAULTS


@pytest.mark.parametrize("var", sorted(VARIABLES))
def test_variable_is_read_by_its_rule(driver, var):
    member, cases = VARIABLES[var]
    for value, want in cases.items():
        got = env(driver, None if value is None else {var: value})
        expect = dict(DEFAULTS)
        expect[member] = DEFAULTS[member] if want == "default" else want
        assert got == expect, (var, value)


def test_the_cases_of_the_issue(driver):
    def one(var, value, member):
        return env(driver, None if value is None else {var: value})[member]
    assert [one("BLSMI_MSM_SORT", v, "msm_sort") for v in (None, "0", "00", "1", "no")] == [1, 0, 0, 1, 1]
    assert [one("BLSMI_HASH_G2_PAIR", v, "hash_g2_pair") for v in (None, "0", "2", "yes")] == [1, 0, 1, 0]
    assert [one("BLSMI_DUP_FORCE_SORT", v, "dup_force_sort") for v in (None, "0", "1")] == [0, 1, 1]
    assert [one("BLSMI_MUL_GENERIC", v, "mul_subgroup") for v in (None, "0", "1", "00")] == [1, 1, 0, 0]
    assert [one("BLSMI_LAYOUT", v, "pair_layout") for v in ("single", "pair", None)] == [0, 1, 1]
    assert [one("BLSMI_GEN_LINES", v, "use_gen_lines") for v in ("0", "00")] == [0, 1]
    assert [one("BLSMI_SIG_SIDE_MAX", v, "sig_side_max") for v in ("-1", "100")] == [-1, 100]
    got = env(driver, {"BLSMI_ROW_MIN": "1024", "BLSMI_ROW_MAX": "0"})
    assert (got["row_min"], got["row_max"]) == (1024, 0)
    assert {k: v for k, v in got.items() if k not in ("row_min", "row_max")} == {k: v for k, v in DEFAULTS.items() if k not in ("row_min", "row_max")}


def test_a_row_set_through_the_api_is_not_touched_by_its_variable(driver):
    variables = {"BLSMI_ROW_MIN": "1024", "BLSMI_ROW_MAX": "0", "BLSMI_MSM_SORT": "0", "BLSMI_LAYOUT": "single"}
    got = env(driver, variables, explicit=("row_max", "msm_sort"))
    assert (got["row_min"], got["row_max"], got["msm_sort"], got["pair_layout"]) == (1024, 8192, 1, 0)
    for var, (member, cases) in VARIABLES.items():                         # every row, each with a value that would move it
        value = next(v for v, want in cases.items() if v is not None and want != "default" and want != DEFAULTS[member])
        assert env(driver, {var: value})[member] != DEFAULTS[member], var
        assert env(driver, {var: value}, explicit=(member,)) == DEFAULTS, var


CHILD = r"""
import ctypes, json, sys
from bls_amd import _native
lib = _native.load()
lib.blsmi_set_option.argtypes = [ctypes.c_char_p, ctypes.c_longlong]
names = json.loads(sys.argv[1])
print(json.dumps([lib.blsmi_set_option(None if n is None else n.encode(), 1) for n in names]))
"""


def test_set_option_accepts_exactly_the_run_time_names():
    """In a child process, so that the options of the test session's own library stay as they are.  Before initialisation, no device."""
    from bls_amd import _native
    _native.build()
    names = RUNTIME_NAMES + ["pair_layout", "swu_wave_max", "quad_min", "", "nope", None, "lat_max", "mul_subgroup", "AGG_COFACTOR_POW", "msm_sort "]
    out = subprocess.run([sys.executable, "-c", CHILD, json.dumps(names)], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    got = dict(zip(names, json.loads(out.splitlines()[-1])))
    BLSMI_E_ARG = -3
    assert got == {n: (0 if n in RUNTIME_NAMES else BLSMI_E_ARG) for n in names}


def test_only_the_table_reads_an_option_s_variable():
    """bls_amd/csrc: every getenv with a literal name reads one of the process's own variables, and no file but route.h names an option's"""
    process = {"BLSMI_COMBINE_MAX", "BLSMI_COMBINE_WAIT_US", "BLSMI_COMBINE_INFLIGHT", "BLSMI_COMBINE_DEBUG", "BLSMI_RCCL_PATH", "BLSMI_STREAMS",
               "BLSMI_SHARDS", "BLSMI_SHARD_MIN", "BLSMI_ARENA_KEEP_MB", "BLSMI_FORCE_RCCL", "BLSMI_DEVICE_ALIAS"}
    csrc = os.path.join(ROOT, "bls_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        if not f.endswith((".hip", ".inc", ".h", ".hpp", ".cuh")):
            continue
        text = "\n".join(l.split("//")[0] for l in open(os.path.join(csrc, f), errors="ignore").read().splitlines())
        for arg in re.findall(r"\bgetenv\(([^)]*)\)", text):
            if arg.startswith('"'):
                assert arg.strip('"') in process, (f, arg)
            else:
                assert f == "blsmi.hip" and arg == "name", (f, arg)         # load_env: its helper for the process's numbers, and apply_env's reader
        for var in VARIABLES:
            assert f == "route.h" or '"%s"' % var not in text, (f, var)
