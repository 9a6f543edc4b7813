"""The inputs of the grouped key partition tests (tests/test_gpu_partition_grouped.py on the GPU, tests/test_partition_group_host.py
without one) and their references (tests/partition_group_ref.py).  Nothing here needs a GPU.

The shapes, rows, queries (qseeds) and filter columns t3 / t64 / distinct / skew are partition_cases' own; what is added is the
GROUP columns.  The condition on the inputs is partition_cases.Case.assert_distinct: all rows are pairwise differently far from
each query, so the position is never consulted and RANGE and IN qualify for the equivalence on the one-list index S1.  The one case
with deliberate ties (tie_groups over partition_cases.tie_case) is held to the reference's (distance, position) order alone."""
import numpy as np

import partition_cases as pc
import partition_group_ref as pgr
from long_rows_cases import wide

EMPTY = 0xFFFFFFFF

# (k, group_size): the distinct forms and the grouped forms; list slots S = 1, 4, 16 in both passes (k, resp. k * group_size, up to
# 64 / 256 / 1024), k * group_size = 1024 both as 512 groups of 2 and as ONE group of 1024
DISTINCT_KM = ((1, 1), (10, 1), (100, 1), (300, 1), (1024, 1))
GROUPED_KM = ((10, 3), (64, 4), (100, 10), (512, 2), (1, 1024))
GROUP_COLUMNS = ("doc32", "doc64", "few", "single")


def group_columns(n, seed):
    """name -> (values int32 / int64 [n], valid bytes or None): the group layouts of the tests.
        doc32   I32, no NULLs: about n / 4 documents of 4 chunks, half the ids negative, assigned by a permutation, so a document's
                chunks are scattered over the filter keys and the inverted lists
        doc64   I64 with 20 % NULLs: the same layout from another permutation, ids beyond the i32 range (wide())
        few     I32: 5 groups, so that n_found < k
        single  I32, no NULLs: every row its own group"""
    rng = np.random.default_rng(seed)
    doc32 = (rng.permutation(n) // 4 - n // 8).astype(np.int32)
    ids = rng.permutation(n) // 4
    doc64 = wide(ids + (ids >= 128)).astype(np.int64)       # (wide(128) = 128 is the one value inside i32: skipped)
    doc64_valid = (rng.random(n) >= 0.2).astype(np.uint8)
    few = (rng.integers(0, 5, n) - 2).astype(np.int32)
    single = (rng.permutation(n) - n // 2).astype(np.int32)
    return {"doc32": (doc32, None), "doc64": (doc64, doc64_valid), "few": (few, None), "single": (single, None)}


class GroupCase(pc.Case):
    """partition_cases.Case plus the group columns and the grouped references"""

    def __init__(self, name, nq=None):
        super().__init__(name, nq)
        self.groups = group_columns(self.n, 5000 + self.dim + 53)

    def grouped(self, part, flt, gcol, k, m, sqrt_out=False, allow=None):
        """partition_group_ref.grouped_batch over this case: part = Case.partition(filter column), flt = one of Case.filters()"""
        _, kind, a, b = flt
        values, valid = self.groups[gcol]
        return pgr.grouped_batch(part[0], part[1], kind, a, b, self.d, values, valid, k, m, self.kind, sqrt_out, allow)


def tie_groups():
    """a 7-valued I32 group column over partition_cases.tie_case()'s rows"""
    n = len(pc.tie_case()[2])
    return np.random.default_rng(41).integers(0, 7, n).astype(np.int32)
