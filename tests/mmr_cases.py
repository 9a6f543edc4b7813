"""The candidate sets of the MMR tests (tests/test_gpu_mmr.py on the GPU, tests/test_mmr_host.py without one) over the inputs of the
key partition tests (partition_cases.SHAPES / LONG_SHAPES: no two rows of a case equally far from a query).  Nothing here needs a
GPU.

n: 1 (one lane), 63 / 64 / 65 (a partial tile, a full one, a second wave's first lane), 257 (a wave with two tiles: tile 4 is wave
0's second) and 1024 (all four tiles of all four waves).  k: 1, 10, n and -- on sets with ids that are no rows -- above the
considered count.  lambda: 0, 0.3, 0.5 and 1."""
import numpy as np

from partition_ref import order_bits, output

EMPTY = 0xFFFFFFFF
NS = (1, 63, 64, 65, 257, 1024)
LAMBDAS = (0.0, 0.3, 0.5, 1.0)


def nearest(d_q, kind, pool, n):
    """the n rows of `pool` nearest by (order bits of d_q, row): a stage 1's order"""
    pool = np.asarray(pool, np.int64)
    return pool[np.lexsort((pool, order_bits(kind, np.asarray(d_q, np.float32)[pool])))[:n]].astype(np.uint32)


def shuffled(cand, seed):
    return np.random.default_rng(seed).permutation(np.asarray(cand, np.uint32))


def with_duplicates(cand, seed):
    """every fifth entry a copy of the first one, every eleventh a copy of a random other"""
    rng = np.random.default_rng(seed)
    c = np.array(cand, np.uint32)
    if len(c):
        at = np.arange(10, len(c), 11)
        c[at] = c[rng.integers(0, len(c), len(at))]
        c[4::5] = c[0]
    return c


def messy(cand, n_rows, seed, removed=()):
    """with_duplicates, and from the fourth entry on every seventh an id that is no row of any list: n_rows, n_rows + 1000,
    0xFFFFFFFF and the `removed` rows in turn"""
    c = with_duplicates(cand, seed)
    junk = [n_rows, n_rows + 1000, EMPTY] + [int(r) for r in removed]
    for j, i in enumerate(range(3, len(c), 7)):
        c[i] = junk[j % len(junk)]
    return c


def rel_of(cand, d_q, kind, sqrt_out):
    """rel of every candidate as a top-k call reports it (the output scale); an id beyond the rows gets 0, a tempting value"""
    cand = np.asarray(cand, np.int64)
    d_q = np.asarray(d_q, np.float32)
    ok = cand < len(d_q)
    out = np.zeros(len(cand), np.float32)
    with np.errstate(all="ignore"):
        out[ok] = output(kind, d_q[cand[ok]], sqrt_out)
    return out


def batch(sets, d, kind, sqrt_out):
    """-> (cand u32 [nq, n], rel f32 [nq, n]) of per-query candidate arrays of one length"""
    cand = np.stack([np.asarray(c, np.uint32) for c in sets])
    return cand, np.stack([rel_of(c, d[q], kind, sqrt_out) for q, c in enumerate(cand)])


# the hand-written case of test_mmr_host.py: 6 rows in 2 dims, the query at the origin
HAND_ROWS = np.array([[1, 0], [1, 1], [-2, 0], [0, 3], [2, 2], [3, 0]], np.float32)
HAND_INDEXED = np.array([1, 1, 1, 1, 0, 1], bool)           # row 4 is in no list
HAND_CAND = np.array([0, 1, 0, 2, 4, 3, 5], np.uint32)      # row 0 twice, the unindexed row 4 at position 4
HAND_REL = np.array([1, 2, 1, 4, 8, 9, 9], np.float32)      # d2 to the origin
HAND_N_FOUND_IN = 6                                         # position 6 (row 5) is beyond it
