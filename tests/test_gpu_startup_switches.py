"""-m gpu: the start-up switches of include/blsmi.h ("A/B switches between code paths with identical results": BLSMI_LAYOUT,
BLSMI_GEN_LINES, BLSMI_MSM_BUCKET_MIN, BLSMI_HASH_G1_SPLIT, BLSMI_SWU_WAVE_MAX, BLSMI_FIXED_WAVE_MAX, BLSMI_SIG_SIDE_MAX,
BLSMI_SIDE_MAX) held to the oracle.  They are Set::fixed rows of the option table (route.h): read once, when the library initialises,
so every configuration is one fresh child process -- this file is its own worker, as in test_gpu_hash_pair.py -- started with
subprocess.run under a time limit, one after the other.

The parent builds one seeded workload and every expected answer with the oracle alone (oracle.refcpu, oracle.pyref) and never
initialises the GPU; the child reads the workload from a file, builds none of its inputs on the device, and prints after each call the
outputs (per record: raw hex where the output is small, a SHA-256 digest otherwise) and the kernel names of blsmi_last_profile.  The
parent compares EVERY record of every output with the oracle -- bit for bit, no sample, no comparison between children -- and checks the
kernel names that prove the switch took effect (the prof_mark strings of blsmi.hip / verify_host.inc).

n = 67 throughout: the layouts put 64, 32, 16 and 4 tuples in a workgroup, so every layout has a full workgroup and a ragged last one,
and the last tuple of each verify batch is a bad one.

Two things the profile cannot show, by construction (prof_mark records on the call's own stream):
  * the signature side's k_miller1s_row of a Verify in the row layout runs on a side stream and is not in the log; k_miller1m_row -- the
    kernel that multiplies that side's values in, launched only when the side kernel was -- is what a Verify's profile names.  The
    aggregate's k_miller1s_row (launch_miller1) is on the call's stream and is named.
  * BLSMI_SIDE_MAX=0 by itself leaves Deserialize + Verify on three streams for n <= the latency threshold (verify_host.inc:
    n <= max(lat_max, side_max)); the one-stream path needs the latency threshold below n as well, so that child runs the call both ways.

A child that dies (signal, abort, time limit, HIP's illegal-memory-access error) sets a module-level latch: every later child of the
module fails at once without starting a process, naming the first casualty.  A child that merely prints wrong values sets no latch.

Measured: the oracle fixture takes 3.6 to 9 s on one CPU core (two hosts); on one MI355X the default configuration's child takes 1.1 s of
wall time (interpreter start and library initialisation included; 0.64 s inside the worker) and no child more than 1.3 s, hence
CHILD_LIMIT_S = 60: ten times that, and at least 60 s.  The limit is a safety net, not a performance claim."""
import ctypes
import hashlib
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 67
DOMAIN = bytes([1, 2, 3, 4, 5, 6, 7, 8])
CHILD_LIMIT_S = 60

# the bad tuples of every verify batch
I_KEY, I_MSG, I_SIG, I_FLAG, I_ZERO, I_LAST = 5, 17, 33, 40, 50, N - 1
I_NONCANON = 7                                                             # serialized batch: a signature whose x is not below the modulus

# ---- thresholds a child sets before a group of calls ("forced": as the fixtures of test_gpu_verify.py / test_gpu_row.py select a layout) ----
#                  latency, quad, (row min, row max), row_side_g2pubs, msm_sort
SETTINGS = {
    "default":    (8192, 16384, (2048, 8192), 1, 1),
    "pair":       (0, 0, (0, 0), 1, 1),                                    # lane pair -- or, under BLSMI_LAYOUT=single, one tuple per lane
    "quad":       (0, 16384, (0, 0), 1, 1),
    "row":        (8192, 16384, (1, 1 << 20), 1, 1),                       # the signature side beside the hash
    "row-noside": (8192, 16384, (1, 1 << 20), 0, 1),                       # g2pubs: the two-pair loop k_miller2_row
    "nosort":     (8192, 16384, (2048, 8192), 1, 0),                       # the MSM's exact digit passes instead of the sort
}

PAIRING = ["pairing", "pprod", "miller"]
VERIFY = ["g2v", "g1v", "g1vd"]
G2AGG = ["g2agg_ok", "g2agg_bad", "g2common_ok", "g2common_bad"]
G1AGG = ["g1agg_ok", "g1agg_bad"]
MSM_CASES = ["n1", "n2", "n67", "cancel"]
MSM_G1 = ["msm_g1_%s%s" % (c, a) for a in ("", "_any") for c in MSM_CASES]
MSM_G2 = ["msm_g2_%s%s" % (c, a) for a in ("", "_any") for c in MSM_CASES]
EVERYTHING = PAIRING + VERIFY + G2AGG + G1AGG + ["g2mul", "g2mul_any"] + MSM_G1 + MSM_G2 + ["hash_g1", "hash_g2", "gen1", "gen2", "ser_g2"]
NOT_WIDE = ("_pair", "_quad", "_row")


def _only_one_lane(names):
    """BLSMI_LAYOUT=single: no Miller loop or final exponentiation of a wider layout"""
    return [k for k in names if k.startswith(("k_miller", "k_final_exp")) and k.endswith(NOT_WIDE)]


def _no_waves(names):
    """BLSMI_SWU_WAVE_MAX=0: no one-wave-per-exponentiation kernel"""
    return [k for k in names if k.endswith(("_waves", "_waves8"))]


def _no(*banned):
    return lambda names: [k for k in names if k in banned]


# configuration -> (environment, [(settings, calls)], [(settings, call, kernel names that must appear)], [(settings, calls, names -> offenders)])
CONFIGS = {
    "defaults": ({}, [("pair", EVERYTHING), ("default", ["gen1", "gen2"] + VERIFY)],          # the control: same worker, same expectations
                 [("pair", "pairing", ["k_miller1h_pair", "k_final_exp_pair"]), ("pair", "miller", ["k_miller1_pair"]), ("pair", "g2v", ["k_miller2_pair", "k_final_exp_is_one_pair"]),
                  ("pair", "g2mul", ["k_g2_mul_glv_pair"]), ("pair", "msm_g1_n67", ["k_g1_mul_glv"]), ("pair", "msm_g2_n67", ["k_g2_mul_glv_pair"]),
                  ("default", "gen1", ["k_g1_mul_fixed_wave"]), ("default", "gen2", ["k_g2_mul_fixed_wave"]),
                  ("default", "g2v", ["k_swu_g1_waves", "k_lat:verify2"]), ("default", "g1v", ["k_swu_g2_waves", "k_lat:verify1s"]), ("default", "g1vd", ["k_lat:verify1s"])], []),
    "single": ({"BLSMI_LAYOUT": "single"}, [("pair", EVERYTHING)],
               [("pair", c, ["k_miller2", "k_final_exp_is_one"]) for c in VERIFY + ["ser_g2"]]
               + [("pair", "pairing", ["k_miller1h", "k_final_exp"]), ("pair", "pprod", ["k_miller1h", "k_final_exp"]), ("pair", "miller", ["k_miller1"]),
                  ("pair", "g2agg_ok", ["k_miller1h"]), ("pair", "g1agg_ok", ["k_miller1h"]),
                  ("pair", "g2mul", ["k_g2_mul_glv"]), ("pair", "g2mul_any", ["k_g2_mul"]), ("pair", "msm_g2_n67", ["k_g2_mul_glv"])],
               [("pair", PAIRING + VERIFY + G2AGG + G1AGG + ["ser_g2"], _only_one_lane), ("pair", ["g2mul", "g2mul_any"] + MSM_G2, _no("k_g2_mul_glv_pair", "k_g2_mul_pair"))]),
    "single-gen-lines-0": ({"BLSMI_LAYOUT": "single", "BLSMI_GEN_LINES": "0"}, [("pair", ["g2v"] + G2AGG)],
                           [("pair", "g2v", ["k_miller2", "k_final_exp_is_one"]), ("pair", "g2agg_ok", ["k_miller1h"])],
                           [("pair", ["g2v"] + G2AGG, _only_one_lane)]),
    "gen-lines-0": ({"BLSMI_GEN_LINES": "0"},
                    [("pair", ["g2v"]), ("quad", ["g2v"]), ("row", ["g2v"]), ("row-noside", ["g2v"]), ("pair", G2AGG), ("row", G2AGG)],
                    [("pair", "g2v", ["k_miller2_pair"]), ("quad", "g2v", ["k_miller2_quad"]), ("row", "g2v", ["k_miller1m_row"]),
                     ("row-noside", "g2v", ["k_miller2_row"]), ("pair", "g2agg_ok", ["k_miller1x2_pair"]), ("row", "g2agg_ok", ["k_miller1s_row"])], []),
    "msm-bucket-min-1": ({"BLSMI_MSM_BUCKET_MIN": "1"}, [("default", MSM_G1 + MSM_G2), ("pair", MSM_G1 + MSM_G2), ("nosort", MSM_G1 + MSM_G2)],
                         [(s, "msm_g1_" + c, ["k_g1_msm_bucket_raw", "k_g1_msm_chunk2", "k_g1_msm_fold2", tail % 1] + digits) for s, tail, digits in
                          (("default", "k_lat:msmfin%d", ["rocprim:radix_sort"]), ("pair", "k_g%d_msm_final2", ["rocprim:radix_sort"]), ("nosort", "k_lat:msmfin%d", ["k_msm_scatter_glv"])) for c in MSM_CASES]
                         + [(s, "msm_g2_" + c, ["k_g2_msm_bucket_raw_pair", "k_g2_msm_chunk2_pair", "k_g2_msm_fold2_pair", tail % 2] + digits) for s, tail, digits in
                            (("default", "k_lat:msmfin%d", ["rocprim:radix_sort"]), ("pair", "k_g%d_msm_final2", ["rocprim:radix_sort"]), ("nosort", "k_lat:msmfin%d", ["k_msm_scatter_glv"])) for c in MSM_CASES]
                         + [(s, "msm_g1_%s_any" % c, ["k_g1_msm_bucket", "k_g1_msm_chunk", "k_g1_msm_fold", "k_g1_msm_final"]) for s in ("default", "pair", "nosort") for c in MSM_CASES]
                         + [(s, "msm_g2_%s_any" % c, ["k_g2_msm_bucket_pair", "k_g2_msm_chunk", "k_g2_msm_fold", "k_g2_msm_final"]) for s in ("default", "pair", "nosort") for c in MSM_CASES], []),
    "msm-bucket-min-1-single": ({"BLSMI_MSM_BUCKET_MIN": "1", "BLSMI_LAYOUT": "single"}, [("default", MSM_G2), ("pair", MSM_G2), ("nosort", MSM_G2)],
                                [(s, "msm_g2_" + c, ["k_g2_msm_bucket_raw_pair", "k_g2_msm_chunk2", "k_g2_msm_fold2", tail]) for s, tail in
                                 (("default", "k_lat:msmfin2"), ("pair", "k_g2_msm_final2"), ("nosort", "k_lat:msmfin2")) for c in MSM_CASES]
                                + [(s, "msm_g2_%s_any" % c, ["k_g2_msm_bucket", "k_g2_msm_chunk", "k_g2_msm_fold", "k_g2_msm_final"]) for s in ("default", "pair", "nosort") for c in MSM_CASES],
                                [(s, MSM_G2, _no("k_g2_msm_chunk2_pair", "k_g2_msm_fold2_pair", "k_g2_msm_bucket_pair")) for s in ("default", "pair", "nosort")]),
    "hash-g1-split-0": ({"BLSMI_HASH_G1_SPLIT": "0"}, [("pair", ["hash_g1", "g2v"])],
                        [("pair", "hash_g1", ["k_hash_g1"]), ("pair", "g2v", ["k_hash_g1", "k_miller2_pair"])],
                        [("pair", ["hash_g1", "g2v"], _no("k_swu_g1_two_lanes", "k_swu_g1_rows", "k_swu_g1_waves", "k_hash_g1_finish"))]),
    "swu-wave-max-0": ({"BLSMI_SWU_WAVE_MAX": "0"}, [("default", ["hash_g1", "hash_g2"] + VERIFY)],
                       [("default", "hash_g1", ["k_swu_g1_rows", "k_lat:hashfin1"]), ("default", "hash_g2", ["k_swu_g2_rows", "k_lat:hashfin2"]),
                        ("default", "g2v", ["k_swu_g1_rows"]), ("default", "g1v", ["k_swu_g2_rows"]), ("default", "g1vd", ["k_tai_g2_lanes8"])],
                       [("default", ["hash_g1", "hash_g2"] + VERIFY, _no_waves)]),
    "fixed-wave-max-0": ({"BLSMI_FIXED_WAVE_MAX": "0"}, [("default", ["gen1", "gen2"])],
                         [("default", "gen1", ["k_g1_mul_fixed"]), ("default", "gen2", ["k_g2_mul_fixed"])],
                         [("default", ["gen1", "gen2"], _no("k_g1_mul_fixed_wave", "k_g2_mul_fixed_wave"))]),
    "sig-side-max-0": ({"BLSMI_SIG_SIDE_MAX": "0"}, [("default", VERIFY)],
                       [("default", c, ["k_lat:verify2"]) for c in VERIFY], [("default", VERIFY, _no("k_lat:verify1s"))]),
    "sig-side-max-large": ({"BLSMI_SIG_SIDE_MAX": "1048576"}, [("default", VERIFY)],
                           [("default", c, ["k_lat:verify1s"]) for c in VERIFY], [("default", VERIFY, _no("k_lat:verify2"))]),
    "side-max-0": ({"BLSMI_SIDE_MAX": "0"}, [("default", ["ser_g2"]), ("pair", ["ser_g2"])],
                   [("default", "ser_g2", ["k_lat:verify2"]), ("pair", "ser_g2", ["k_miller2_pair"])], []),
}


# ---- what both sides share: packing, the printed form of an output --------------------------------------------------------------------
def _pack(msgs):
    off = np.zeros(len(msgs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs])
    return np.frombuffer(b"".join(msgs) or b"\0", dtype=np.uint8), off


def _unpack(buf, off):
    b = buf.tobytes()
    return [b[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


def _tokens(a, nrec):
    """one token per record: the record's hex where the whole output is small (or a record is a flag), its SHA-256 otherwise"""
    a = np.ascontiguousarray(a).view(np.uint8).reshape(nrec, -1)
    raw = a.size <= 256 or a.shape[1] <= 8
    return [r.tobytes().hex() if raw else hashlib.sha256(r.tobytes()).hexdigest() for r in a]


def _point(p, nbytes):
    """a single point (None: infinity) as an output field"""
    return ["inf"] if p is None else _tokens(np.frombuffer(p, dtype=np.uint8), 1)


def _points(pts, nbytes):
    """points with None for infinity -> the (records, flags) an entry point returns: zero bytes and flag 1 there"""
    rec = np.zeros((len(pts), nbytes), dtype=np.uint8)
    for i, p in enumerate(pts):
        if p is not None:
            rec[i] = np.frombuffer(p, dtype=np.uint8)
    return {"out": _tokens(rec, len(pts)), "inf": _tokens(np.array([p is None for p in pts], dtype=np.uint8), len(pts))}


# ---- the child ------------------------------------------------------------------------------------------------------------------------
def _calls(E, W):
    """call name -> function returning {field: tokens}; every input comes from the workload file"""
    msgs, msgs32 = _unpack(W["msgs_buf"], W["msgs_off"]), [r.tobytes() for r in W["msgs32"]]
    agg, agg_bad = _unpack(W["agg_buf"], W["agg_off"]), _unpack(W["aggbad_buf"], W["aggbad_off"])
    g1, g2, ks = W["g1"].tobytes(), W["g2"].tobytes(), W["scalars"].tobytes()

    def verdicts(ok, bitmap=None):
        d = {"ok": _tokens(np.asarray(ok, dtype=np.uint8), N)}
        if bitmap is not None:
            d["bitmap"] = _tokens(bitmap, 1)
        return d

    def one(ok):
        return {"ok": ["%02x" % int(bool(ok))]}

    def mul(res):
        out, inf = res
        return {"out": _tokens(out, out.shape[0]), "inf": _tokens(inf.astype(np.uint8), out.shape[0])}

    def pprod():
        vals, is_one = E.pairing_product_batch(g1, g2, E.seg_offsets([0, 1, N - 1]))
        return {"values": _tokens(vals, 3), "is_one": _tokens(is_one, 3)}

    def ser():
        ok, ep, es = E.verify_serialized_batch("g2pubs", msgs, W["ser_pkc"].tobytes(), W["ser_sgc"].tobytes())
        return {"ok": _tokens(ok.astype(np.uint8), N), "err_pk": _tokens(ep, N), "err_sig": _tokens(es, N)}

    c = {
        "pairing": lambda: {"values": _tokens(E.pairing_batch(g1, g2, N), N)},
        "pprod": pprod,
        "miller": lambda: {"values": _tokens(E.miller_loop_batch(g1, g2, N), N)},
        "g2v": lambda: verdicts(*E.g2pubs_verify_batch(msgs, W["g2v_pks"].tobytes(), W["g2v_sigs"].tobytes(), W["g2v_flags"])),
        "g1v": lambda: verdicts(*E.g1pubs_verify_batch(msgs, W["g1v_pks"].tobytes(), W["g1v_sigs"].tobytes(), W["g1v_flags"])),
        "g1vd": lambda: verdicts(E.g1pubs_verify_with_domain_batch(msgs32, DOMAIN, W["g1vd_pks"].tobytes(), W["g1vd_sigs"].tobytes(), W["g1vd_flags"])),
        "g2agg_ok": lambda: one(E.g2pubs_verify_aggregate(agg, W["g2agg_pks"].tobytes(), W["g2agg_sig"].tobytes())),
        "g2agg_bad": lambda: one(E.g2pubs_verify_aggregate(agg_bad, W["g2agg_pks"].tobytes(), W["g2agg_sig"].tobytes())),
        "g1agg_ok": lambda: one(E.g1pubs_verify_aggregate(agg, W["g1agg_pks"].tobytes(), W["g1agg_sig"].tobytes())),
        "g1agg_bad": lambda: one(E.g1pubs_verify_aggregate(agg_bad, W["g1agg_pks"].tobytes(), W["g1agg_sig"].tobytes())),
        "g2common_ok": lambda: one(E.g2pubs_verify_aggregate_common(agg[0], W["g2agg_pks"].tobytes(), W["g2common_sig"].tobytes(), N)),
        "g2common_bad": lambda: one(E.g2pubs_verify_aggregate_common(agg[0], W["g2agg_pks"].tobytes(), W["g2common_sig_bad"].tobytes(), N)),
        "g2mul": lambda: mul(E.g2_mul_batch(W["pts2"].tobytes(), ks, N)),
        "g2mul_any": lambda: mul(E.g2_mul_batch(W["pts2"].tobytes(), ks, N, any_point=True)),
        "hash_g1": lambda: {"points": _tokens(E.hash_g1_batch(msgs), N)},
        "hash_g2": lambda: {"points": _tokens(E.hash_g2_batch(msgs), N)},
        "gen1": lambda: mul(E.g1_mul_generator_batch(ks, N)),
        "gen2": lambda: mul(E.g2_mul_generator_batch(ks, N)),
        "ser_g2": ser,
    }
    for grp, fn, nb in (("g1", E.g1_msm, 96), ("g2", E.g2_msm, 192)):
        for case in MSM_CASES:
            pts, sc = (W["cancel_" + grp], W["cancel_scalars"]) if case == "cancel" else (W["pts1" if grp == "g1" else "pts2"][:int(case[1:])], W["scalars"][:int(case[1:])])
            for any_point in (False, True):
                c["msm_%s_%s%s" % (grp, case, "_any" if any_point else "")] = \
                    lambda fn=fn, pts=pts, sc=sc, nb=nb, a=any_point: {"sum": _point(fn(pts.tobytes(), sc.tobytes(), pts.shape[0], any_point=a), nb)}
    return c


def _worker(path, key):
    t0 = time.time()
    sys.path.insert(0, ROOT)
    from bls_amd import engine as E
    W = dict(np.load(path))
    E.init(0)
    lib = E._lib()
    lib.blsmi_set_profiling(1)
    buf = ctypes.create_string_buffer(1 << 16)

    def profile():
        lib.blsmi_last_profile(buf, ctypes.c_size_t(len(buf)))
        return [item.rsplit("=", 1)[0].replace(" ", "_") for item in buf.value.decode().split(";") if item]

    calls = _calls(E, W)
    for settings, names in CONFIGS[key][1]:
        lat, quad, row, side_g2pubs, msm_sort = SETTINGS[settings]
        E.set_latency_threshold(lat); E.set_quad_threshold(quad); E.set_row_threshold(*row)
        E.set_option("row_side_g2pubs", side_g2pubs); E.set_option("msm_sort", msm_sort)
        for name in names:
            profile()                                                      # forget what came before (initialisation, the previous call)
            t = time.time()
            fields = calls[name]()
            for field, tokens in fields.items():
                print("OUT %s/%s %s %s" % (settings, name, field, " ".join(tokens)), flush=True)
            print("PROF %s/%s %s" % (settings, name, " ".join(profile())), flush=True)
            print("TIME %s/%s %.3f" % (settings, name, time.time() - t), flush=True)
    print("WALL %.2f" % (time.time() - t0), flush=True)                    # nothing is restored: the process ends here


# ---- the parent: workload and expectations from the oracle, on the CPU ---------------------------------------------------------------
def _neg1(p):
    return p[:48] + ((-int.from_bytes(p[48:], "big")) % _Q()).to_bytes(48, "big")


def _neg2(p):
    return p[:96] + b"".join(((-int.from_bytes(p[o:o + 48], "big")) % _Q()).to_bytes(48, "big") for o in (96, 144))


def _Q():
    from gpu_common import P
    return P.Q


def _build():
    """-> (arrays of the workload file, {call: {field: tokens}} from the oracle)"""
    from gpu_common import P, RC, rand_g1, rand_g2, sk_bytes
    xs = P.XORShift(20261018)
    rng = np.random.default_rng(20261018)
    W, X = {}, {}
    arr = lambda recs: np.frombuffer(b"".join(recs), dtype=np.uint8).reshape(len(recs), -1).copy()   # noqa: E731
    G1, G2 = RC.g1_generator(), RC.g2_generator()

    # messages: the SHA-256 padding boundaries with the hash's one-byte prefix, then seeded lengths up to 150; all distinct
    lens = [0, 1, 55, 56, 119, 120] + [int(l) for l in rng.integers(2, 151, size=N - 6)]
    msgs = [bytes(rng.integers(0, 256, size=l, dtype=np.uint8)) for l in lens]
    assert len(set(msgs)) == N
    msgs32 = [hashlib.sha256(b"with domain %d" % i).digest() for i in range(N)]
    W["msgs_buf"], W["msgs_off"] = _pack(msgs)
    W["msgs32"] = arr(msgs32)

    # Pairing, pairing products in segments of 0, 1 and 66
    g1s, g2s = [rand_g1(xs) for _ in range(N)], [rand_g2(xs) for _ in range(N)]
    W["g1"], W["g2"] = arr(g1s), arr(g2s)
    X["pairing"] = {"values": _tokens(RC.pairing_batch(b"".join(g1s), b"".join(g2s), N), N)}
    X["miller"] = {"values": _tokens(np.stack([RC.miller_loop(a, b, 1) for a, b in zip(g1s, g2s)]), N)}     # MillerLoop: the reference's exact steps
    one = np.zeros(72, dtype=np.uint64); one[:6] = np.array(P.limbs64(P.to_mont(1)), dtype=np.uint64)
    vals = [one]
    for lo, hi in ((0, 1), (1, N)):
        ok, v = RC.final_exponentiation(RC.miller_loop(b"".join(g1s[lo:hi]), b"".join(g2s[lo:hi]), hi - lo))
        assert ok
        vals.append(v)
    X["pprod"] = {"values": _tokens(np.array(vals, dtype=np.uint64), 3), "is_one": _tokens(np.array([np.array_equal(v, one) for v in vals], dtype=np.uint8), 3)}

    # Verify x 67 with the six bad tuples.  The library takes the all-zero record for the point at infinity and gives such a tuple, like a
    # flagged one, verdict 0 (the reference panics there): the oracle is told so through its flags.
    sks = [sk_bytes(xs) for _ in range(N)]
    keys = {RC.g2pubs: [RC.g2pubs.priv_to_pub(sk) for sk in sks], RC.g1pubs: [RC.g1pubs.priv_to_pub(sk) for sk in sks]}
    for kind, o, ms, pkb, rand_sig, flag in (("g2v", RC.g2pubs, msgs, 192, rand_g1, 1), ("g1v", RC.g1pubs, msgs, 96, rand_g2, 2), ("g1vd", RC.g1pubs, msgs32, 96, rand_g2, 1)):
        sign = (lambda m, sk: RC.g1pubs.sign_with_domain(m, sk, DOMAIN)) if kind == "g1vd" else o.sign
        pks, sigs = list(keys[o]), [sign(m, sk) for m, sk in zip(ms, sks)]
        pks[I_KEY] = o.priv_to_pub(sk_bytes(xs))
        sigs[I_MSG] = sign(ms[I_MSG][:-1] + bytes([ms[I_MSG][-1] ^ 1]), sks[I_MSG])
        sigs[I_SIG] = rand_sig(xs)
        sigs[I_LAST] = sign(ms[I_LAST] + b"!" if kind != "g1vd" else msgs32[0], sks[I_LAST])
        pks[I_ZERO] = bytes(pkb)
        flags = np.zeros(N, dtype=np.uint8); flags[I_FLAG] = flag
        oflags = flags.copy(); oflags[I_ZERO] |= 1
        if kind == "g1vd":
            want = np.array([not oflags[i] and RC.g1pubs.verify_with_domain(ms[i], pks[i], sigs[i], DOMAIN) for i in range(N)], dtype=np.uint8)
        else:
            want = o.verify_batch(ms, pks, sigs, oflags).astype(np.uint8)
        bad = {I_KEY, I_MSG, I_SIG, I_FLAG, I_ZERO, I_LAST}
        assert [i for i in range(N) if not want[i]] == sorted(bad), (kind, want)            # the workload is what it claims to be
        W[kind + "_pks"], W[kind + "_sigs"], W[kind + "_flags"] = arr(pks), arr(sigs), flags
        X[kind] = {"ok": _tokens(want, N)}
        if kind != "g1vd":
            X[kind]["bitmap"] = _tokens(np.packbits(want, bitorder="little"), 1)
        if kind == "g2v":
            g2v = (pks, sigs, want)

    # VerifyAggregate over 67 distinct messages (odd: the last tuple has no partner in the two-tuple loops): valid, and one message changed
    agg = [b"aggregate message %d" % i for i in range(N)]
    agg_bad = list(agg); agg_bad[N // 2] = b"aggregate message %d?" % (N // 2)
    W["agg_buf"], W["agg_off"] = _pack(agg)
    W["aggbad_buf"], W["aggbad_off"] = _pack(agg_bad)
    for grp, o, summ in (("g2", RC.g2pubs, RC.g1_sum), ("g1", RC.g1pubs, RC.g2_sum)):
        pks = keys[o]
        sig = summ(b"".join(o.sign(m, sk) for m, sk in zip(agg, sks)), N)
        W[grp + "agg_pks"], W[grp + "agg_sig"] = arr(pks), arr([sig])
        X[grp + "agg_ok"] = {"ok": ["%02x" % o.verify_aggregate(sig, pks, agg)]}
        X[grp + "agg_bad"] = {"ok": ["%02x" % o.verify_aggregate(sig, pks, agg_bad)]}
        if grp == "g2":                                                    # VerifyAggregateCommon: 67 keys, one message; invalid: a signature missing
            csigs = [o.sign(agg[0], sk) for sk in sks]
            for tag, part in (("", csigs), ("_bad", csigs[1:])):
                cs = summ(b"".join(part), len(part))
                W["g2common_sig" + tag] = arr([cs])
                X["g2common_" + ("bad" if tag else "ok")] = {"ok": ["%02x" % o.verify_aggregate_common(cs, pks, agg[0])]}
    assert X["g2agg_ok"]["ok"] == X["g1agg_ok"]["ok"] == X["g2common_ok"]["ok"] == ["01"] and X["g2agg_bad"]["ok"] == X["g1agg_bad"]["ok"] == X["g2common_bad"]["ok"] == ["00"]

    # scalar multiples, PrivToPub, multi-scalar multiplication: a random scalar and r - 1 first (the n = 1 and n = 2 sums), then 0, 1, r, r + 1,
    # 2^256 - 1, a scalar twice, random ones
    R = P.R_ORDER
    ks = [sk_bytes(xs) for _ in range(N)]
    for i, v in enumerate((R - 1, 0, 1, R, R + 1, (1 << 256) - 1)):
        ks[1 + i] = v.to_bytes(32, "big")
    ks[9] = ks[8]
    pts1, pts2 = [rand_g1(xs) for _ in range(N)], [rand_g2(xs) for _ in range(N)]
    W["scalars"], W["pts1"], W["pts2"] = arr(ks), arr(pts1), arr(pts2)
    m1, m2 = [RC.g1_mul(p, k) for p, k in zip(pts1, ks)], [RC.g2_mul(p, k) for p, k in zip(pts2, ks)]
    assert [i for i in range(N) if m2[i] is None] == [2, 4] == [i for i in range(N) if m1[i] is None]
    X["g2mul"] = X["g2mul_any"] = _points(m2, 192)
    gen1, gen2 = [RC.g1_mul(G1, k) for k in ks], [RC.g2_mul(G2, k) for k in ks]
    for i in range(N):                                                     # PrivToPub is the generator's multiple
        assert gen1[i] is None or gen1[i] == RC.g1pubs.priv_to_pub(ks[i])
        assert gen2[i] is None or gen2[i] == RC.g2pubs.priv_to_pub(ks[i])
    X["gen1"], X["gen2"] = _points(gen1, 96), _points(gen2, 192)
    W["cancel_g1"], W["cancel_g2"] = arr([pts1[0], _neg1(pts1[0])]), arr([pts2[0], _neg2(pts2[0])])
    W["cancel_scalars"] = arr([ks[0], ks[0]])
    for grp, mults, summ, nb, cancel in (("g1", m1, RC.g1_sum, 96, W["cancel_g1"]), ("g2", m2, RC.g2_sum, 192, W["cancel_g2"])):
        mul = RC.g1_mul if grp == "g1" else RC.g2_mul
        for case in MSM_CASES:
            part = [mul(cancel[i].tobytes(), ks[0]) for i in range(2)] if case == "cancel" else mults[:int(case[1:])]
            part = [p for p in part if p is not None]
            want = summ(b"".join(part), len(part)) if part else None
            assert (want is None) == (case == "cancel")
            X["msm_%s_%s" % (grp, case)] = X["msm_%s_%s_any" % (grp, case)] = {"sum": _point(want, nb)}

    X["hash_g1"] = {"points": _tokens(arr([RC.hash_g1(m) for m in msgs]), N)}
    X["hash_g2"] = {"points": _tokens(arr([RC.hash_g2(m) for m in msgs]), N)}

    # Deserialize + Verify over the compressed g2pubs tuples: the infinity encoding where the affine batch had the flag and the zero record, and a
    # signature whose x is the modulus itself.  Expected as tests/test_gpu_verify.py::test_verify_serialized_batch derives it: the oracle's error
    # codes, and verdict 0 wherever an element fails to deserialise or is the point at infinity; elsewhere the oracle's verdict on what it decoded.
    pks, sigs, _ = g2v
    pkc = [RC.g2_compress(None if i == I_ZERO else p) for i, p in enumerate(pks)]
    sgc = [RC.g1_compress(None if i == I_FLAG else s) for i, s in enumerate(sigs)]
    b = bytearray(P.Q.to_bytes(48, "big")); b[0] |= 0x80; sgc[I_NONCANON] = bytes(b)
    dp, ds = [RC.g2_decompress(c) for c in pkc], [RC.g1_decompress(c) for c in sgc]
    assert ds[I_NONCANON][0] != 0 and dp[I_ZERO] == (0, None) and ds[I_FLAG] == (0, None)
    want = np.array([p is not None and s is not None and RC.g2pubs.verify(msgs[i], p, s) for i, ((_, p), (_, s)) in enumerate(zip(dp, ds))], dtype=np.uint8)
    assert [i for i in range(N) if not want[i]] == sorted({I_KEY, I_MSG, I_SIG, I_FLAG, I_ZERO, I_LAST, I_NONCANON})
    W["ser_pkc"], W["ser_sgc"] = arr(pkc), arr(sgc)
    X["ser_g2"] = {"ok": _tokens(want, N), "err_pk": _tokens(np.array([e for e, _ in dp], dtype=np.uint8), N), "err_sig": _tokens(np.array([e for e, _ in ds], dtype=np.uint8), N)}
    assert set(X) == set(EVERYTHING)
    return W, X


@pytest.fixture(scope="module")
def workload(tmp_path_factory):
    t0 = time.time()
    W, X = _build()
    path = str(tmp_path_factory.mktemp("startup_switches") / "workload.npz")
    np.savez(path, **W)
    print("oracle fixture: %.1f s" % (time.time() - t0))
    return path, X


_first_casualty = None                                                     # the latch: set by the first child that dies, never cleared


def _run(key, path):
    """one fresh child for configuration `key` -> (its stdout lines, its stderr); fails at once when an earlier child of the module died"""
    global _first_casualty
    if _first_casualty:
        pytest.fail("not started: %s" % _first_casualty, pytrace=False)
    env = {k: v for k, v in os.environ.items() if not k.startswith("BLSMI_") or k == "BLSMI_LIB"}
    env.update(CONFIGS[key][0])
    cmd = [sys.executable, os.path.abspath(__file__), path, key]
    try:
        out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=CHILD_LIMIT_S)
    except subprocess.TimeoutExpired as e:
        _first_casualty = "the child of configuration `%s` passed its time limit of %d s" % (key, CHILD_LIMIT_S)
        pytest.fail(_first_casualty + "\n" + str(e.stderr or "")[-2000:], pytrace=False)
    faulted = "illegal memory access" in out.stdout + out.stderr
    if out.returncode < 0 or out.returncode in (134, 139, 124, 137) or faulted:
        _first_casualty = "the child of configuration `%s` %s (status %d)" % (key, "reported an illegal memory access" if faulted else "died", out.returncode)
        pytest.fail(_first_casualty + "\n" + out.stderr[-2000:], pytrace=False)
    assert out.returncode == 0, "configuration `%s`: status %d\n%s" % (key, out.returncode, out.stderr[-2000:])
    return out.stdout.splitlines()


def _mismatch(what, got, want):
    if len(got) != len(want):
        return "%s: %d records, the oracle has %d" % (what, len(got), len(want))
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    if bad:
        return "%s differs from the oracle at index %s%s (%d of %d records): got %s, expected %s" % (
            what, bad[:8], " ..." if len(bad) > 8 else "", len(bad), len(want), got[bad[0]], want[bad[0]])
    return None


def _judge(key, lines, X):
    """every record of every output of every planned call against the oracle, then the kernel names"""
    _, plan, need, ban = CONFIGS[key]
    outs, profs = {}, {}
    for l in lines:
        w = l.split(" ")
        if w[0] == "OUT":
            outs.setdefault(w[1], {})[w[2]] = [t for t in w[3:] if t]
        elif w[0] == "PROF":
            profs[w[1]] = [t for t in w[2:] if t]
    planned = ["%s/%s" % (s, c) for s, calls in plan for c in calls]
    assert sorted(outs) == sorted(planned) == sorted(profs), "configuration `%s`: calls %s missing from the child's output" % (key, sorted(set(planned) - set(outs)))
    errors = []
    for call in planned:
        want = X[call.split("/")[1]]
        assert sorted(outs[call]) == sorted(want), (call, sorted(outs[call]), sorted(want))
        for field in want:
            e = _mismatch("%s %s.%s" % (key, call, field), outs[call][field], want[field])
            if e:
                errors.append(e)
    for s, c, names in need:
        missing = [k for k in names if k not in profs["%s/%s" % (s, c)]]
        if missing:
            errors.append("%s %s/%s: kernels %s not in the profile %s" % (key, s, c, missing, profs["%s/%s" % (s, c)]))
    for s, calls, offenders in ban:
        for c in calls:
            bad = offenders(profs["%s/%s" % (s, c)])
            if bad:
                errors.append("%s %s/%s: kernels %s in the profile %s" % (key, s, c, bad, profs["%s/%s" % (s, c)]))
    return errors


@pytest.mark.parametrize("key", list(CONFIGS))
def test_startup_switch_against_the_oracle(key, workload):
    path, X = workload
    lines = _run(key, path)
    print("\n".join(l for l in lines if l.startswith(("WALL", "TIME"))))
    errors = _judge(key, lines, X)
    assert not errors, "\n".join(errors)


if __name__ == "__main__":
    _worker(sys.argv[1], sys.argv[2])
