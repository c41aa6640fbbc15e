"""What tests/test_pprod_rlc_locate_cpu.py and tests/test_gpu_pprod_rlc_locate.py share (blsmi 0.18: blsmi_pairing_product_batch_rlc_locate*),
over the corpus of tests/pprod_rlc_corpus.py: the blocks of a batch, the block values from the oracle alone, and what `rechecked` must be."""
import numpy as np

from oracle import refcpu as RC
from pprod_rlc_corpus import ONE, Corpus

BAD1, BAD2 = (2,), (7, 21)                                                      # as tests/test_gpu_pprod_rlc.py: a Groth16-shaped item; an item of the two-item entry and a two-pair item
BLOCKS = (0, 1, 8, 33, 64)


def auto_block(m):
    return max(64, -(-m // 256))


def blocks_of(m, block):
    """[(lo, hi)] of the B = ceil(m / block) contiguous blocks; block 0: the automatic rule"""
    block = block or auto_block(m)
    return [(lo, min(m, lo + block)) for lo in range(0, m, block)]


def rechecked_of(m, block, bad):
    """the summed sizes of the blocks with an item of `bad` in them"""
    return sum(hi - lo for lo, hi in blocks_of(m, block) if any(lo <= j < hi for j in bad))


def block_value(c, r, lo, hi):
    """FE(prod over the cells of the block of items [lo, hi) of Miller(S_c, Q_g(c))) from the oracle's primitives: the block on its own is a
    batch whose groups are its cells, so this is Corpus.combined_value over those items alone (infinite pairs add nothing, an all-zero entry
    drops its cell, a cell whose sum is infinity contributes 1, no surviving cell: one)"""
    sub = Corpus(items=[])
    sub.items = c.items[lo:hi]
    return sub.combined_value(r[lo:hi])


def is_one(v):
    return bool(np.array_equal(np.asarray(v, dtype=np.uint64), ONE))


def fq12_prod(vs):
    out = ONE
    for v in vs:
        out = RC.fq12_mul(out, v)
    return out
