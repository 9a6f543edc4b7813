"""The candidate lists of the candidate-list tests (tests/test_gpu_rows.py on the GPU, tests/test_rows_host.py without one) over the
inputs of the key partition tests (partition_cases.SHAPES / LONG_SHAPES: no two rows of a case equally far from a query).  Nothing
here needs a GPU.

Slice lengths: 0, 1, 63, 64, 65, 255, 256, 257 -- around a wave's 64-position window and a block's turn of 256 -- and 1000 / 1003, which
a block walks in several turns (partition_blocks 1: four; 2: two).  Five queries take them in two batches (LENS_A, LENS_B)."""
import numpy as np

EMPTY = 0xFFFFFFFF
LENS_A = (0, 1, 63, 64, 1000)
LENS_B = (65, 255, 256, 257, 1003)
KS = (1, 10, 64, 65, 1024)


def unique_lists(n, lens, seed, ascending=False):
    """one list per length: distinct rows of [0, n), in random order (ascending: sorted)"""
    rng = np.random.default_rng(seed)
    out = [rng.choice(n, ln, replace=False).astype(np.uint32) for ln in lens]
    return [np.sort(l) for l in out] if ascending else out


def messy_lists(n, lens, seed, bound=None):
    """one list per length, unsorted, with what a caller's list may hold: rows drawn WITH replacement (duplicates), every fifth entry
    a copy of the list's first one, and -- from the fourth entry on, every seventh -- an id that is no row: n, n + 1000, `bound`
    (where given) or 0xFFFFFFFF in turn"""
    rng = np.random.default_rng(seed)
    junk = [n, n + 1000, EMPTY] + ([bound] if bound is not None else [])
    out = []
    for ln in lens:
        l = rng.integers(0, n, ln).astype(np.uint32)
        l[4::5] = l[0] if ln else 0
        for j, i in enumerate(range(3, ln, 7)):
            l[i] = junk[j % len(junk)]
        out.append(l)
    return out
