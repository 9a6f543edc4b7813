"""The inputs of the partition range search tests (tests/test_gpu_partition_range.py on the GPU, tests/test_partition_range_host.py
without one) and their references (tests/partition_range_ref.py).  Nothing here needs a GPU.

Shapes: partition_cases' -- the four of pc.SHAPES with their key columns (t3, t64, distinct, skew) and EQ / RANGE / IN filters, and
through long_rows_cases.Case "768", "134-dot", "132-cos" and "260" -- whose inputs have no two rows equally far from a query, plus:

    BIG       10 000 x 24, one key of 9 000 rows, 3 queries: nothing in pc.SHAPES exceeds 4096 rows, and 4096 is what ONE block sorts
              (RANGE_SMALL).  More than 8 192 hits at +inf: two merge passes; under a 50 % mask more than 4 096: one; max_results cuts
              inside the segment.  Integer-valued rows: many EQUAL distances, so the (distance key, position) order is consulted all
              the way down.  Compared with the restatement only.
    tie_case  pc.tie_case(): deliberate ties under a 4-valued key.

Radii are DERIVED from the reference per (case, filter, mask, output scale), never hard-coded (radii()): one below every considered
distance (no hit), +inf (every considered row), the upper median of the pooled considered distances (itself a distance: inclusive),
and exactly the distance of the BOUNDARY_J-th nearest considered row of query 0 -- with distinct distances n_within[0] == j + 1.
PQV_DOT distances are negative on these inputs (rows and queries in [0, 1)), so every finite radius of a dot case is negative."""
import numpy as np

import key_filter_ref as kf
import long_rows_cases as lrc
import partition_cases as pc
import partition_range_ref as prr
import partition_ref as pr

SHAPES = pc.SHAPES
LONG_SHAPES = pc.LONG_SHAPES
COLUMNS = ("t3", "t64", "distinct", "skew")
BLOCKS = pc.BLOCKS
BOUNDARY_J = 7
RANGE_SMALL = 4096                      # csrc/kernels.h: the hits one block sorts; longer segments are merged in passes of 2 x
BIG = dict(n=10000, dim=24, nq=3, big_key=1, big_rows=9000, seed=8123)
BIG_MAX_RESULTS = (1, 4096, 4097, 9000)


def radii(ref_inf):
    """[(label, radius f32)] from the reference at radius = +inf (prr.range_batch's tuple, distances on the output scale)"""
    lims, _, dist = ref_inf[:3]
    inf = np.float32(np.inf)
    pooled = np.sort(dist[~np.isnan(dist)])
    if len(pooled) == 0:
        return [("below", np.float32(-1.0)), ("inf", inf)]
    out = [("below", np.nextafter(pooled[0], -inf)), ("inf", inf), ("median", pooled[len(pooled) // 2])]
    n0 = int(lims[1])
    if n0:
        j = min(BOUNDARY_J, n0 - 1)
        out.append((f"boundary{j}", dist[j]))
    return out


def boundary_j(label):
    return int(label[len("boundary"):]) if label.startswith("boundary") else None


class LongCase:
    """A long_rows_cases shape as the partition tests read it: rows, queries, the distance matrix, two key columns -- the I32 tenant
    keys with NULLs and the same keys widened to I64 without -- and their EQ / RANGE / IN filters"""

    def __init__(self, name, oracle):
        lc = self.lc = lrc.Case(name, oracle)
        self.name, self.n, self.dim, self.kind, self.metric, self.nq = name, lc.n, lc.dim, lc.kind, lc.metric, lrc.NQ
        self.data, self.queries = lc.data, lc.queries
        self.d = pr.distances(lc.kind, lc.metric, lc.data, lc.queries)
        self.shared = lc.masks["1/2"]
        lims, vals = kf.sets_to_csr(lrc.QUERY_SETS)
        self.columns, self._filters = {}, {}
        for col, values, valid, conv in (("i32", lc.tenant, lc.tenant_valid, lambda v: [int(x) for x in v]),
                                         ("i64", lrc.wide(lc.tenant), None, lambda v: [int(x) for x in lrc.wide(v)])):
            self.columns[col] = (values, valid)
            self._filters[col] = [("eq", kf.EQ, conv(lrc.QUERY_KEYS), None),
                                  ("range", kf.RANGE, conv(lrc.QUERY_RANGES[0]), conv(lrc.QUERY_RANGES[1])),
                                  ("in", kf.IN, [int(x) for x in lims], conv(vals) if len(vals) else [])]

    def filters(self, col):
        return self._filters[col]

    def partition(self, col, indexed=None):
        values, valid = self.columns[col]
        return pr.build(values, valid, np.arange(self.n) if indexed is None else indexed)


def reference(case, part, flt, radius, sqrt_out=False, allow=None, max_results=0):
    """prr.range_batch of a pc.Case / LongCase / BigCase"""
    _, kind, a, b = flt
    return prr.range_batch(part[0], part[1], kind, a, b, case.d, radius, case.kind, sqrt_out, allow, max_results)


class BigCase:
    """BIG: integer-valued rows under an I32 key whose value big_key holds big_rows of the n rows"""

    def __init__(self):
        c = BIG
        rng = np.random.default_rng(c["seed"])
        self.name, self.n, self.dim, self.nq, self.kind, self.metric = "big", c["n"], c["dim"], c["nq"], "l2", pr.REF4
        self.data = rng.integers(0, 4, (self.n, self.dim)).astype(np.float32)
        self.queries = rng.integers(0, 4, (self.nq, self.dim)).astype(np.float32)
        keys = rng.integers(2, 12, self.n).astype(np.int32)
        keys[rng.permutation(self.n)[:c["big_rows"]]] = c["big_key"]
        self.keys = keys
        self.columns = {"key": (keys, None)}
        self.shared = rng.random(self.n) < 0.5
        self.d = pr.distances("l2", pr.REF4, self.data, self.queries)
        lims, vals = kf.sets_to_csr([[1, 3], [1], [2, 3, 4]])
        self._filters = [("eq", kf.EQ, [1, 1, 5], None), ("range", kf.RANGE, [kf.INT64_MIN, 1, 2], [kf.INT64_MAX, 1, 11]),
                         ("in", kf.IN, [int(x) for x in lims], [int(x) for x in vals])]
        # four lists, rows dealt round: the partition order (key, row) is not the list order
        self.lists = [np.arange(i, self.n, 4, dtype=np.uint32) for i in range(4)]

    def filters(self, col="key"):
        return self._filters

    def partition(self, col="key", indexed=None):
        return pr.build(self.keys, None, np.arange(self.n) if indexed is None else indexed)


class TieCase:
    """pc.tie_case() as a case: (data, queries, keys int32), three lists dealt round, the filters of the top-k tie test"""

    def __init__(self):
        self.data, self.queries, self.keys = pc.tie_case()
        self.name, (self.n, self.dim), self.nq, self.kind, self.metric = "ties", self.data.shape, len(self.queries), "l2", pr.REF4
        self.columns = {"key": (self.keys, None)}
        self.d = pr.distances("l2", pr.REF4, self.data, self.queries)
        lims, vals = kf.sets_to_csr([[0, 3], [1], [0, 1, 2, 3], [2, 9], []])
        self._filters = [("eq", kf.EQ, [0, 1, 2, 3, 7], None), ("range", kf.RANGE, [0, 1, 0, 3, 2], [1, 3, 3, 3, 1]),
                         ("in", kf.IN, [int(x) for x in lims], [int(x) for x in vals])]
        self.lists = [np.arange(i, self.n, 3, dtype=np.uint32) for i in range(3)]

    def filters(self, col="key"):
        return self._filters

    def partition(self, col="key", indexed=None):
        return pr.build(self.keys, None, np.arange(self.n) if indexed is None else indexed)
