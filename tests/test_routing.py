"""Which kernels a call runs, without a GPU: bls_amd/csrc/route.h compiled into a small driver (tests/native/route_table.cc) and asked
at the boundaries of every hand-over.  The tables are the routing of the library before route.h existed, with one intended change:
prepared keys follow the call's layout (a prepared call in the row range gathers its keys and runs the row kernels)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    gpp = shutil.which("g++")
    if gpp is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("route") / "route_table")
    subprocess.check_call([gpp, "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "route_table.cc")])

    def run(question, sizes, kind=0, others=0, **opts):
        tail = "".join(" %s=%d" % kv for kv in sorted(opts.items()))
        text = "".join("%s %d %d %d%s\n" % (question, kind, n, others, tail) for n in sizes)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(sizes)
        return dict(zip(sizes, out))
    return run


def table(**ranges):
    """{n: answer} from answer=(sizes...) keyword groups"""
    return {n: k for k, ns in ranges.items() for n in ns}


def test_pairing_layout_at_defaults(ask):
    want = table(wave=(1, 2047), row=(2048, 8192, 8193, 12288), quad=(12289, 16384), pair=(16385, 65536))
    assert ask("pairing", list(want)) == want


def test_verify_layout_at_defaults(ask):
    want = table(wave=(1, 320, 1000, 2047), row=(2048, 4096, 8192), quad=(8193, 12288, 16384), pair=(16385, 65536))
    assert ask("verify", list(want)) == want


def test_miller_loop_and_final_exp_layouts(ask):
    assert ask("miller", [1, 8192, 8193]) == {1: "wave", 8192: "wave", 8193: "pair"}
    assert ask("final_exp", [2047, 2048, 8192, 8193]) == {2047: "wave", 2048: "row", 8192: "row", 8193: "single"}
    assert ask("final_exp", [1, 8192, 8193], lat_max=1024, row_max=0) == {1: "wave", 8192: "single", 8193: "single"}


def test_aggregate_layout_and_records(ask):
    want = {1: "wave 1", 2047: "wave 2047", 2048: "row 2048", 8192: "row 8192", 8193: "quad 4097", 32768: "quad 16384",
            32769: "pair 16385", 65536: "pair 32768"}
    assert ask("aggregate", list(want)) == want
    # a latency threshold below the row range: up to it a wave per tuple, above two tuples per lane quad
    assert ask("aggregate", [1024, 1025, 4096], lat_max=1024) == {1024: "wave 1024", 1025: "quad 513", 4096: "quad 2048"}
    assert ask("aggregate", [8192, 8193], pair_layout=0) == {8192: "wave 8192", 8193: "single 8193"}


def test_crowded_calls(ask):
    # 2 048 tuples with 4 096 others in flight: past the lone crossover together, the quad kernels; alone, the row kernels
    assert ask("verify", [2048], others=4096) == {2048: "quad"}
    assert ask("pairing", [2048], others=4096) == {2048: "quad"}
    assert ask("verify", [2048], assume_load=4096) == {2048: "quad"}
    # below the crowd floor (1 536) the load is not looked at
    assert ask("verify", [1000, 1535], others=100000) == {1000: "wave", 1535: "wave"}
    assert ask("verify", [1536], others=100000) == {1536: "quad"}
    assert ask("verify", [2048, 5632], others=4096, crowd_quad=0) == {2048: "row", 5632: "row"}


def test_settings_move_the_hand_overs(ask):
    assert ask("verify", [1024, 1025, 2048, 8193], lat_max=1024) == {1024: "wave", 1025: "quad", 2048: "row", 8193: "quad"}
    assert ask("verify", [5632, 5633, 16385], row_max=0) == {5632: "wave", 5633: "quad", 16385: "pair"}
    assert ask("verify", [2048, 8192, 8193], quad_max=0) == {2048: "row", 8192: "row", 8193: "pair"}
    assert ask("pairing", [8193, 12288, 12289], quad_max=0) == {8193: "row", 12288: "row", 12289: "pair"}
    assert ask("verify", [1, 8192, 8193], pair_layout=0) == {1: "wave", 8192: "wave", 8193: "single"}


def test_signature_side(ask):
    assert ask("side", [1, 48, 49, 2047, 2048, 8192, 8193, 16385], kind=0) == table(
        wave=(1, 48), none=(49, 2047, 8193, 16385), row=(2048, 8192))
    assert ask("side", [320, 321, 2048, 8192], kind=1) == {320: "wave", 321: "none", 2048: "row", 8192: "row"}
    assert ask("side", [4096], kind=0, row_side_g2pubs=0) == {4096: "none"}
    assert ask("side", [4096], kind=1, row_side_g2pubs=0) == {4096: "row"}
    assert ask("side", [4096, 48], kind=0, row_side=0) == {4096: "none", 48: "wave"}
    assert ask("side", [10, 100, 101], kind=1, sig_side_max=100) == {10: "wave", 100: "wave", 101: "none"}
    assert ask("side", [2048], kind=0, others=4096) == {2048: "none"}   # crowded into the quad layout: no side stream


def test_prepared_tables(ask):
    # columns: Verify, Pairing, VerifyAggregate
    want = {8192: "0 0 0", 16384: "0 0 0", 16385: "1 1 0", 32768: "1 1 0", 32769: "1 1 1", 65536: "1 1 1"}
    assert ask("prepared", list(want)) == want
    assert ask("prepared", [65536], use_gen_lines=0) == {65536: "0 1 0"}
    # the intended change: a latency threshold below the row range no longer sends a row-range call to the lane-pair prepared kernels
    assert ask("prepared", [2048, 4096, 8192, 8193], lat_max=1024) == {2048: "0 0 0", 4096: "0 0 0", 8192: "0 0 0", 8193: "0 0 0"}
    assert ask("prepared", [16385], lat_max=1024) == {16385: "1 1 0"}


def test_hash_tails_at_their_edges(ask):
    # HashG2 (g1pubs): the eight-lane tail 2 048 .. 7 168, the four-lane tail up to 16 384, a lane pair above; the smallest on the level programs
    g2 = ask("hash", [1, 512, 513, 2047, 2048, 7168, 7169, 16384, 16385], kind=1)
    assert g2 == {1: "lat waves", 512: "lat waves", 513: "lat rows", 2047: "lat rows", 2048: "g2_oct lanes", 7168: "g2_oct lanes",
                  7169: "g2_quad lanes", 16384: "g2_quad lanes", 16385: "g2_pair lanes"}
    assert ask("hash", [2048, 4096, 4097], kind=1, hash_oct_max=0) == {2048: "g2_row lanes", 4096: "g2_row lanes", 4097: "g2_quad lanes"}
    assert ask("hash", [3072, 3073], kind=1, hash_oct_max=0, hash_row_max=0, hash_quad_max=0) == {3072: "lat rows", 3073: "g2_pair lanes"}
    # HashG1 (g2pubs): the four-lane tail 1 280 .. 32 768 behind the two-lane maps (maps a row each up to swu_row_max, a lane each beside the side kernel)
    g1 = ask("hash", [1279, 1280, 2047, 2048, 4096, 4097, 32768, 32769], kind=0)
    assert g1 == {1279: "lat rows", 1280: "g1_quad rows", 2047: "g1_quad rows", 2048: "g1_quad lanes", 4096: "g1_quad lanes",
                  4097: "g1_quad lanes", 32768: "g1_quad lanes", 32769: "plain lanes"}
    assert ask("hash", [2048], kind=0, row_side=0) == {2048: "g1_quad rows"}
    assert ask("hash", [3584, 3585], kind=0, hash_g1_quad_max=0, row_side=0) == {3584: "lat rows", 3585: "g1_lane rows"}
    assert ask("hash", [1279], kind=0, swu_row_max=0) == {1279: "lat lanes"}
    # HashG2WithDomain: waves up to a quarter of BLSMI_SWU_WAVE_MAX, eight lanes a message beyond (the row layout: up to 3 072 messages)
    assert ask("hash", [128, 129, 3072, 3073], kind=2) == {128: "lat waves", 129: "lat lanes", 3072: "lat lanes", 3073: "plain lanes"}
    # a g2pubs aggregate that raises its product to 1 - x hashes without clearing the cofactor: never the level programs or the four-lane tail
    assert ask("hash_agg", [100, 32768, 32769], kind=0) == {100: "g1_lane lanes", 32768: "g1_lane lanes", 32769: "plain lanes"}


def test_tuple_blocks(ask):
    """the workgroups of n tuples: 64, 32, 16 and 4 tuples to a workgroup of 64 lanes in the single, pair, quad and row layouts"""
    sizes = sorted({n for per in (64, 32, 16, 4) for n in (0, 1, per - 1, per, per + 1, 2 ** 20 + 1)})
    want = {n: "%d %d %d %d" % ((n + 63) // 64, (n + 31) // 32, (n + 15) // 16, (n + 3) // 4) for n in sizes}
    assert ask("blocks", sizes) == want
