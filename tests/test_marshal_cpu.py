"""Every public wrapper of bls_amd.engine marshals its arguments without a device: each one is called on zero-filled inputs (host forms with
n = 0 and n = 2, device-pointer forms with pointer 0 and n = 0, and once with each optional argument present) and must end as
tests/golden/marshal_outcomes.json records it: a normal return with its shapes and dtypes, BlsmiError with its code, or ValueError.
ctypes.ArgumentError or TypeError anywhere is a failure.  The file was recorded before the binding was derived from the header
(`python tests/test_marshal_cpu.py --record` rewrites it); the made-up pointers must never reach a device, so the module skips where one is."""
import ctypes
import inspect
import json
import os
import re
import sys

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "marshal_outcomes.json")
EXEMPT = {"BlsmiError", "PackedMsgs", "seg_offsets"}                     # pure helpers and classes: no C call behind them
Z = bytes
D8 = bytes(8)
FAKE = 4096                                                              # a made-up device pointer


def M(n):
    return [bytes(3)] * n


def M32(n):
    return [bytes(32)] * n


def _rows(engine):
    """(wrapper, label, args, kwargs) for every case; a keyword replaces the positional argument of its name"""
    R = []

    def add(name, label, *a, **k):
        R.append((name, label, a, k))

    def host(name, args, tag="", **opts):
        """args(n) -> the positional arguments; opts: label = kwargs(n), one extra call each at n = 2"""
        for n in (0, 2):
            add(name, "%sn%d" % (tag, n), *args(n))
        for label, kw in opts.items():
            add(name, tag + label, *args(2), **kw(2))

    def dev(name, *args, tag="", **opts):
        tag = tag or (args[0] + "_" if isinstance(args[0], str) else "")
        add(name, tag + "null", *args)
        for label, kw in opts.items():
            add(name, tag + label, *args, **kw)

    inf = dict(inf_flags=lambda n: dict(inf_flags=Z(n)))
    in_inf = dict(in_inf=lambda n: dict(in_inf=Z(n)))
    sc = dict(scalars=lambda n: dict(scalars=[1] * n))
    blk = dict(block=lambda n: dict(block=2))
    anyp = dict(any_point=lambda n: dict(any_point=True))
    # ---- process-wide calls (defaults, so that nothing changes for the tests that follow)
    add("init", "dev0")
    add("init_devices", "all")
    add("debug_alias_own", "null", 0, 0, 0)
    add("trim", "zero")
    add("held_bytes", "now")
    for shape, n in ((5, 1), (5, 100), (0, 1)):
        add("prefer_cpu", "shape%d_n%d" % (shape, n), shape, n)
    add("device_leases", "dev0", 0)
    add("device_count", "now")
    add("shard_count", "now")
    add("set_latency_threshold", "default", 8192)
    add("set_quad_threshold", "default", 16384)
    add("set_row_threshold", "default", 2048, 8192)
    add("set_option", "msm_sort", "msm_sort", 1)
    add("set_option", "unknown", "no_such_option", 1)
    add("set_mul_assume_subgroup", "default", True)
    add("version", "now")
    add("HostBuffer", "n0", 0)
    add("HostBuffer", "n64", 64)
    add("shutdown", "now")
    # ---- pairing
    host("pairing_batch", lambda n: (Z(96 * n), Z(192 * n), n), out=lambda n: dict(out=np.zeros((n, 72), np.uint64)))
    host("miller_loop_batch", lambda n: (Z(96 * n), Z(192 * n), n))
    host("final_exponentiation_batch", lambda n: (np.zeros((n, 72), np.uint64),))
    host("fq12_product", lambda n: (np.zeros((n, 72), np.uint64),))
    host("g2_prepare_batch", lambda n: (Z(192 * n), n))
    host("PreparedKeys", lambda n: (Z(192 * n), n))
    host("PreparedKeysJac", lambda n: (Z(288 * n), n))
    host("pairing_batch_jac", lambda n: (Z(144 * n), Z(288 * n), n))
    host("pairing_product_batch", lambda n: (Z(96 * n), Z(192 * n), [0, n] if n else [0]), **inf)
    host("pairing_product_batch_jac", lambda n: (Z(144 * n), Z(288 * n), [0, n] if n else [0]))
    dev("pairing_batch_dev", 0, 0, 0, 0)
    dev("pairing_batch_jac_dev", 0, 0, 0, 0)
    dev("pairing_batch_prepared_dev", 0, 0, 0, 0, 0)
    dev("g2_prepare_batch_dev", 0, 0, 0)
    dev("g2_prepared_export_dev", 0, 0, 0)
    dev("pairing_product_batch_dev", 0, 0, 0, 0, 0, 0, 0, jac=dict(jac=True), flags=dict(d_inf_flags=FAKE), jac_flags=dict(jac=True, d_inf_flags=FAKE))
    # ---- groups
    for g, pb in (("g1", 96), ("g2", 192)):
        host(g + "_mul_batch", lambda n, pb=pb: (Z(pb * n), Z(32 * n), n), **anyp)
        host(g + "_mul_generator_batch", lambda n: (Z(32 * n), n))
        host(g + "_mul_generator_batch_jac", lambda n: (Z(32 * n), n))
        host(g + "_msm", lambda n, pb=pb: (Z(pb * n), Z(32 * n), n), **anyp)
        host(g + "_sum", lambda n, pb=pb: (Z(pb * n), n), **in_inf)
        host(g + "_sum_jac", lambda n, pb=pb: (Z(pb // 2 * 3 * n), n))
        host(g + "_jac_to_affine_batch", lambda n, pb=pb: (Z(pb // 2 * 3 * n), n))
        host(g + "_decompress_batch", lambda n, pb=pb: (Z(pb // 2 * n), n), check=lambda n: dict(check_subgroup=False))
        host(g + "_compress_batch", lambda n, pb=pb: (Z(pb * n), n), **in_inf)
        host(g + "_decompress_batch_jac", lambda n, pb=pb: (Z(pb // 2 * n), n), check=lambda n: dict(check_subgroup=False))
        host(g + "_compress_batch_jac", lambda n, pb=pb: (Z(pb // 2 * 3 * n), n))
        host(g + "_check_batch", lambda n, pb=pb: (Z(pb * n), n), check=lambda n: dict(check=2), **in_inf)
        host(g + "_check_batch_jac", lambda n, pb=pb: (Z(pb // 2 * 3 * n), n), check=lambda n: dict(check=0))
        seg = lambda n: (None, [0, n] if n else [0])                     # noqa: E731  (idx, seg_off)
        host(g + "_sum_segmented", lambda n, pb=pb: (Z(pb * n), n) + seg(n), idx=lambda n: dict(idx=[1, 0]), **in_inf)
        host(g + "_sum_segmented_jac", lambda n, pb=pb: (Z(pb // 2 * 3 * n), n) + seg(n), idx=lambda n: dict(idx=[1, 0]))
        host(g + "_sum_segmented_u64", lambda n, pb=pb: (Z(pb * n), n, [1] * n) + seg(n), **in_inf)
        dev("mul_batch_dev", g, 0, 0, 0, 0, 0, any_point=dict(any_point=True))
        dev("sum_dev", g, 0, 0, 0, 0)
        dev("msm_dev", g, 0, 0, 0, 0, any_point=dict(any_point=True))
        dev("sum_segmented_dev", g, 0, 0, 0, 0, 0, 0, 0, 0)
        dev("check_batch_dev", g, 0, 0, 0, 0, jac=dict(jac=True), check=dict(check=2))
        dev("decompress_batch_jac_dev", g, 0, 0, 0, 0, 0, check=dict(check_subgroup=False))
        dev("compress_batch_jac_dev", g, 0, 0, 0)
    add("check_batch_dev", "jac_flags", "g1", 0, FAKE, 0, 0, jac=True)
    host("debug_g2_sum_segmented_u64_pair", lambda n: (Z(192 * n), n, [1] * n, None, [0, n] if n else [0]), **in_inf)
    # ---- hash and sign
    host("hash_g1_batch", lambda n: (M(n),))
    host("hash_g2_batch", lambda n: (M(n),))
    host("hash_g2_with_domain_batch", lambda n: (M32(n), D8))
    add("hash_g1_batch", "packed", engine.PackedMsgs(M(2)))
    for sfx in ("", "_jac"):
        host("g2pubs_sign_batch" + sfx, lambda n: (M(n), Z(32 * n)))
        host("g1pubs_sign_batch" + sfx, lambda n: (M(n), Z(32 * n)))
        host("g1pubs_sign_with_domain_batch" + sfx, lambda n: (M32(n), D8, Z(32 * n)))
    # ---- verify: the wire format and in-memory twins; g2pubs keys are G2 points, g1pubs keys G1 points
    for sfx, k in (("", 2), ("_jac", 3)):                                # bytes per coordinate pair: 96 -> 96 / 144
        P = {"g2pubs": (96 * k, 48 * k), "g1pubs": (48 * k, 96 * k)}    # (key bytes, signature bytes)
        fl = inf if not sfx else {}
        for g, (pkb, sgb) in P.items():
            host(g + "_verify_batch" + sfx, lambda n, pkb=pkb, sgb=sgb: (M(n), Z(pkb * n), Z(sgb * n)), **fl)
            host(g + "_verify_batch_rlc" + sfx, lambda n, pkb=pkb, sgb=sgb: (M(n), Z(pkb * n), Z(sgb * n)), **fl, **sc)
            host(g + "_verify_batch_rlc_locate" + sfx, lambda n, pkb=pkb, sgb=sgb: (M(n), Z(pkb * n), Z(sgb * n)), **fl, **sc, **blk)
            host(g + "_verify_batch_rlc_grouped" + sfx, lambda n, pkb=pkb, sgb=sgb: (M(1 if n else 0), [0] * n, Z(pkb * n), Z(sgb * n)), **fl, **sc)
            host(g + "_verify_batch_rlc_grouped_locate" + sfx, lambda n, pkb=pkb, sgb=sgb: (M(1 if n else 0), [0] * n, Z(pkb * n), Z(sgb * n)), **fl, **sc, **blk)
            host(g + "_verify_aggregate" + sfx, lambda n, pkb=pkb, sgb=sgb: (M(n), Z(pkb * n), Z(sgb)))
            host(g + "_verify_aggregate_common" + sfx, lambda n, pkb=pkb, sgb=sgb: (bytes(3), Z(pkb * n), Z(sgb), n))
            add(g + "_verify_aggregate_common" + sfx, "empty_msg", b"", Z(pkb * 2), Z(sgb), 2)
            # committees: m = n / 2 items over n keys
            host(g + "_verify_aggregate_common_batch" + sfx, lambda n, pkb=pkb, sgb=sgb: (M(n // 2), Z(pkb * n), n, None, [0, n] if n else [0], Z(sgb * (n // 2))),
                 idx=lambda n: dict(idx=[1, 0]))
            host(g + "_verify_aggregate_common_batch_rlc" + sfx,
                 lambda n, pkb=pkb, sgb=sgb: (M(n // 2), [0] * (n // 2), Z(pkb * n), n, None, [0, n] if n else [0], Z(sgb * (n // 2))), **sc_m)
        pkb, sgb = P["g1pubs"]
        wd = "g1pubs_verify_with_domain_batch"
        host(wd + sfx, lambda n, pkb=pkb, sgb=sgb: (M32(n), D8, Z(pkb * n), Z(sgb * n)), **fl)
        host(wd + "_rlc" + sfx, lambda n, pkb=pkb, sgb=sgb: (M32(n), D8, Z(pkb * n), Z(sgb * n)), **fl, **sc)
        host(wd + "_rlc_locate" + sfx, lambda n, pkb=pkb, sgb=sgb: (M32(n), D8, Z(pkb * n), Z(sgb * n)), **fl, **sc, **blk)
        host(wd + "_rlc_grouped" + sfx, lambda n, pkb=pkb, sgb=sgb: (M32(1 if n else 0), D8, [0] * n, Z(pkb * n), Z(sgb * n)), **fl, **sc)
        host(wd + "_rlc_grouped_locate" + sfx, lambda n, pkb=pkb, sgb=sgb: (M32(1 if n else 0), D8, [0] * n, Z(pkb * n), Z(sgb * n)), **fl, **sc, **blk)
        host("g1pubs_verify_aggregate_with_domain" + sfx, lambda n, pkb=pkb, sgb=sgb: (M32(n), D8, Z(pkb * n), Z(sgb)))
        host("g1pubs_verify_aggregate_common_with_domain" + sfx, lambda n, pkb=pkb, sgb=sgb: (Z(32), D8, Z(pkb * n), Z(sgb), n))
        host("g1pubs_verify_aggregate_common_with_domain_batch" + sfx,
             lambda n, pkb=pkb, sgb=sgb: (Z(32 * (n // 2)), D8, Z(pkb * n), n, None, [0, n] if n else [0], Z(sgb * (n // 2))))
        host("g1pubs_verify_aggregate_common_with_domain_batch_rlc" + sfx,
             lambda n, pkb=pkb, sgb=sgb: (M32(n // 2), D8, [0] * (n // 2), Z(pkb * n), n, None, [0, n] if n else [0], Z(sgb * (n // 2))), **sc_m)
    for g, (pkc, sgc) in (("g2pubs", (96, 48)), ("g1pubs", (48, 96))):
        host("verify_serialized_batch", lambda n, g=g, pkc=pkc, sgc=sgc: (g, M(n), Z(pkc * n), Z(sgc * n)), tag=g + "_", check=lambda n: dict(check_subgroup=False))
        host("aggregate_partial", lambda n, g=g, pkc=pkc: (g, M(n), Z(2 * pkc * n)), tag=g + "_")
        dev("verify_batch_dev", g, 0, 0, 0, 0, 0, 0, 0)
        dev("verify_batch_jac_dev", g, 0, 0, 0, 0, 0, 0)
        dev("verify_aggregate_common_dev", g, 0, 0, bytes(3), Z(2 * sgc), empty_msg=dict(msg=b""))
        dev("verify_aggregate_dev", g, 0, 0, 0, Z(2 * sgc), 0)
        dev("verify_aggregate_common_batch_dev", g, 0, 0, 0, 0, 0, 0, 0, 0, 0)
        dev("verify_aggregate_common_batch_rlc_dev", g, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, scalars=dict(scalars=[]))
    dev("verify_batch_jac_dev", "g1pubs_with_domain", 0, 0, 0, 0, 0, 0)
    add("verify_aggregate_common_dev", "g1pubs_domain", "g1pubs", 0, 0, Z(32), Z(192), domain=D8)
    add("verify_aggregate_common_batch_dev", "g1pubs_domain", "g1pubs", 0, 0, 0, 0, 0, 0, 0, 0, 0, domain=True)
    add("verify_aggregate_common_batch_rlc_dev", "g1pubs_domain", "g1pubs", 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, domain=True)
    dev("g1pubs_verify_with_domain_batch_dev", 0, 0, 0, 0, 0, 0, 0)
    dev("verify_aggregate_with_domain_dev", 0, 0, 0, Z(192), 0)
    # ---- prepared keys (the table is a device pointer: made up for n = 2, nothing for n = 0)
    key_idx = dict(key_idx=lambda n: dict(key_idx=[0] * n))
    host("g2pubs_verify_batch_prepared", lambda n: (M(n), FAKE if n else 0, None, Z(96 * n)), **key_idx, **inf)
    host("g2pubs_verify_aggregate_prepared", lambda n: (M(n), FAKE if n else 0, None, Z(96)), **key_idx)
    host("g2pubs_verify_batch_prepared_jac", lambda n: (M(n), FAKE if n else 0, None, Z(144 * n)), **key_idx)
    host("g2pubs_verify_aggregate_prepared_jac", lambda n: (M(n), FAKE if n else 0, None, Z(144)), **key_idx)
    dev("g2pubs_verify_batch_prepared_dev", 0, 0, 0, 0, 0, 0, 0, 0)
    dev("g2pubs_verify_aggregate_prepared_dev", 0, 0, 0, 0, Z(96), 0)
    # ---- unit-level device ops
    add("debug_g2_prepare", "generator", None, 2)
    add("debug_g2_prepare", "point", Z(192), 0)
    for kind, rec in ((0, 192), (1, 384)):
        host("debug_hash_tail", lambda n, kind=kind, rec=rec: (kind, Z(rec * n), n), tag="kind%d_" % kind)
    host("debug_hash_redo", lambda n: (0, M(n), Z(n), np.zeros((n, 96), np.uint8)), tag="kind0_")
    host("debug_hash_redo", lambda n: (2, M32(n), Z(n), np.zeros((n, 192), np.uint8), D8), tag="kind2_")
    host("debug_lat_unit", lambda n: (0, np.zeros((n, 16, 15), np.int32), 1), verdict=lambda n: dict(nout=0))
    host("debug_op", lambda n: ("FQ_MUL", np.zeros((n, 6), np.uint64)), b=lambda n: dict(b=np.zeros((n, 6), np.uint64)), lane_pair=lambda n: dict(lane_pair=True),
         raw_flag=lambda n: dict(raw_flag=True))
    # ---- randomised pairing products, scalar-field folds, Groth16
    for sfx, k in (("", 2), ("_jac", 3)):
        fl = inf if not sfx else {}
        q_idx = dict(q_idx=lambda n: dict(q_idx=[0] * n))
        pp = lambda n, k=k: (Z(48 * k * n), Z(96 * k * n), None, [0, n] if n else [0])   # noqa: E731
        host("pairing_product_batch_rlc" + sfx, pp, **fl, **sc_m1, **q_idx)
        host("pairing_product_batch_rlc_locate" + sfx, pp, **fl, **sc_m1, **q_idx, **blk)
        host("groth16_verify_batch" + sfx, lambda n, k=k: (Z(48 * k * 3), Z(96 * k * 3), Z(48 * k * 2 * n), Z(96 * k * n), Z(32 * n), 1), **sc, **blk)
        add("groth16_verify_batch" + sfx, "nin0", Z(48 * k * 2), Z(96 * k * 3), Z(48 * k * 2 * 2), Z(96 * k * 2), None, 0)
        dev("pairing_product_batch_rlc%s_dev" % sfx, 0, 0, 0, 0, 0, 0, 0, 0, scalars=dict(scalars=[]), **({} if sfx else dict(flags=dict(d_inf_flags=FAKE), nosplit=dict(nosplit=True))))
        dev("pairing_product_batch_rlc_locate%s_dev" % sfx, 0, 0, 0, 0, 0, 0, 0, 0, scalars=dict(scalars=[]), block=dict(block=2), **({} if sfx else dict(flags=dict(d_inf_flags=FAKE))))
        dev("groth16_verify_batch%s_dev" % sfx, 0, 0, 0, 0, 0, 0, 0, 0, scalars=dict(scalars=[]), block=dict(block=2))
    host("fr_wsum_segmented_u64", lambda n: (Z(32 * n), 1, [1] * n, [0, n] if n else [0]))
    dev("fr_wsum_segmented_u64_dev", 0, 0, 0, 0, 0, 0)
    return R


sc_m = dict(scalars=lambda n: dict(scalars=[1] * (n // 2)))              # one scalar per item: m = n / 2 committees
sc_m1 = dict(scalars=lambda n: dict(scalars=[1]))                        # ... m = 1 item of n pairs


def _describe(v):
    if isinstance(v, np.ndarray):
        return ["ndarray", str(v.dtype), list(v.shape)]
    if isinstance(v, (bytes, bytearray)):
        return ["bytes", len(v)]
    if isinstance(v, (tuple, list)):
        return [_describe(x) for x in v]
    if v is None or isinstance(v, (bool, int, str, np.integer, np.bool_)):
        return v.item() if isinstance(v, np.generic) else v
    return ["object", type(v).__name__]


def _outcome(engine, name, args, kwargs):
    fn = getattr(engine, name)
    call = dict(inspect.signature(fn).bind_partial(*args).arguments, **kwargs)
    try:
        return ["return", _describe(fn(**call))]
    except engine.BlsmiError as e:
        return ["BlsmiError", int(re.search(r"failed: .* \((-?\d+)\)$", str(e)).group(1))]
    except ValueError as e:
        assert not isinstance(e, ctypes.ArgumentError), (name, e)
        return ["ValueError"]


def _run_all(engine):
    out = {}
    for name, label, args, kwargs in _rows(engine):
        assert label not in out.setdefault(name, {}), (name, label)
        out[name][label] = _outcome(engine, name, args, kwargs)
    return out


@pytest.fixture(scope="module")
def engine():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from bls_amd import _native, engine
    _native.build()
    return engine


def test_every_public_callable_has_a_row(engine):
    public = {n for n, v in vars(engine).items() if callable(v) and not n.startswith("_") and getattr(v, "__module__", None) == engine.__name__}
    covered = {r[0] for r in _rows(engine)}
    assert covered <= public, covered - public
    assert public - covered == EXEMPT, sorted((public - covered) ^ EXEMPT)


def test_every_wrapper_marshals_as_recorded(engine):
    want = json.load(open(GOLDEN))
    got = _run_all(engine)
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    bad = {(k, c): (got[k].get(c), want[k].get(c)) for k in got for c in set(got[k]) | set(want[k]) if got[k].get(c) != want[k].get(c)}
    assert not bad, bad


if __name__ == "__main__" and sys.argv[1:] == ["--record"]:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bls_amd import engine as _engine
    with open(GOLDEN, "w") as f:                                              # one wrapper a line
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, sort_keys=True)) for k, v in sorted(_run_all(_engine).items())) + "\n}\n")
