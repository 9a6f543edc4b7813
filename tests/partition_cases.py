"""The inputs of the key partition tests (tests/test_gpu_partition.py on the GPU, tests/test_partition_host.py without one) and
their references (tests/partition_ref.py).  Nothing here needs a GPU.

Shapes: the four of test_gpu_mask.SHAPES (CG 32, CG 64, unaligned rows with a scalar tail, the SEQ chain) at their own sizes, and --
through long_rows_cases.Case -- "768", "134-dot" and "132-cos" for rows of several chunks, PQV_DOT and PQV_COSINE, and "260", whose
rows the searcher stores zero-padded.

Ties: the data seed is 5000 + dim and every query is drawn from a seed of its own, chosen by a search on the CPU (the first seeds
from 7000 on that qualify) so that for that query the distances of ALL rows are pairwise distinct (Case.assert_distinct, as
long_rows_cases.Case.assert_distinct) -- every call's considered rows are a subset, so no two rows of different keys tie and the
order (distance, position) never consults the position.  That is a condition on the inputs; no comparison has a tolerance.  The
one case with deliberate ties (tie_case) is held to the reference's (distance, position) order alone."""
import numpy as np

import key_filter_ref as kf
import partition_ref as pr
from long_rows_cases import wide
from range_oracle import REF4, SEQ

EMPTY = 0xFFFFFFFF

# name -> n, dim, kc, metric as test_gpu_mask.SHAPES states them (test_partition_host.py compares), and the queries' seeds
SHAPES = {
    "4096x128": dict(n=4096, dim=128, kc=8, metric=REF4, qseeds=[7014, 7023, 7029, 7044, 7061]),
    "2048x256": dict(n=2048, dim=256, kc=4, metric=REF4, qseeds=[7001, 7002, 7003, 7004, 7005]),
    "1500x30": dict(n=1500, dim=30, kc=6, metric=REF4,
                    qseeds=[7000, 7001, 7002, 7003, 7004, 7005, 7006, 7007, 7008, 7009, 7010, 7011, 7013, 7015, 7016, 7017, 7018, 7019, 7021,
                            7023, 7024, 7025, 7026, 7027, 7028, 7029, 7030, 7031, 7032, 7034, 7035, 7036, 7037, 7038, 7039, 7040, 7041, 7042,
                            7043, 7044, 7045, 7046, 7047, 7048, 7049, 7050, 7051, 7052, 7053, 7054, 7055, 7056, 7057, 7058, 7059, 7060, 7062,
                            7063, 7064, 7065, 7066, 7067, 7068, 7070, 7071, 7072, 7073, 7074, 7075, 7076]),
    "2048x32-seq": dict(n=2048, dim=32, kc=4, metric=SEQ, qseeds=[7000, 7001, 7002, 7003, 7004]),
}
LONG_SHAPES = ("768", "134-dot", "132-cos", "260")  # long_rows_cases.SHAPES ("260": stored zero-padded to 320, the queries too)
KS = (1, 10, 100, 300, 1024)
BLOCKS = (1, 3, 0)                                   # the searcher option partition_blocks; 0 = by rule


def draw(name, nq=None):
    """(rows [n, dim], queries [nq, dim]) of a shape: nq <= len(qseeds), the first nq of them"""
    c = SHAPES[name]
    data = np.random.default_rng(5000 + c["dim"]).random((c["n"], c["dim"]), dtype=np.float32)
    seeds = c["qseeds"][:nq] if nq else c["qseeds"]
    return data, np.stack([np.random.default_rng(s).random(c["dim"], dtype=np.float32) for s in seeds])


def columns(n, seed):
    """name -> (values int32 / int64 [n], valid bytes or None): the key layouts of the tests.
        t3        I32, 3 values (runs of ~n / 3 rows: longer than a block's turn of 256), one of them negative
        t64       I64 with NULLs, 64 values beyond the i32 range (wide()), negative for small ones
        distinct  I32 with NULLs, all keys different (runs of one), half of them negative
        skew      I64, one key with more than 512 rows, the rest singletons"""
    rng = np.random.default_rng(seed)
    t3 = np.array([-5, 0, 7], np.int32)[rng.integers(0, 3, n)]
    t64 = wide(rng.integers(0, 64, n))
    t64_valid = (rng.random(n) >= 0.2).astype(np.uint8)
    distinct = (rng.permutation(n) - n // 2).astype(np.int32)
    distinct_valid = (rng.random(n) >= 0.1).astype(np.uint8)
    skew = (np.arange(n, dtype=np.int64) + 1) * np.int64(3)
    skew[rng.permutation(n)[:600]] = np.int64(2 ** 40)
    return {"t3": (t3, None), "t64": (t64.astype(np.int64), t64_valid), "distinct": (distinct, distinct_valid), "skew": (skew, None)}


def filters(col, nq, seed):
    """[(label, kind, a, b)] over the column `col` of columns(): per-query arguments for nq queries.  a / b are lists of Python
    integers (IN: lims and values in the descriptor's CSR form)."""
    rng = np.random.default_rng(seed)
    cyc = lambda vals: [int(vals[i % len(vals)]) for i in range(nq)]     # noqa: E731
    big_set = lambda present, absent: sorted(set(present) | set(absent))    # noqa: E731

    def csr(sets):
        lims, vals = kf.sets_to_csr(sets)
        return [int(x) for x in lims], [int(x) for x in vals]

    out = []
    if col == "t3":
        # 3 is no key of the column; 2^31 and -2^31 - 1 are outside i32 on this I32 column
        out.append(("eq", kf.EQ, cyc([-5, 7, 3, 2 ** 31, -2 ** 31 - 1]), None))
        out.append(("range", kf.RANGE, cyc([-5, 1, 7, kf.INT64_MIN, 2 ** 31]), cyc([0, 6, -5, kf.INT64_MAX, 2 ** 40])))
        out.append(("in", kf.IN, *csr([[[0], [-5, 7], [], [3, 7, 2 ** 31], [-5, -4, 0, 1, 7]][i % 5] for i in range(nq)])))
    elif col == "t64":
        present = [int(x) for x in wide(np.arange(64))]
        out.append(("eq", kf.EQ, cyc([present[0], present[63], present[17], 5, present[0] + 1]), None))
        out.append(("range", kf.RANGE, cyc([present[3], present[10], kf.INT64_MIN, present[40], 0]),
                    cyc([present[3], present[20], kf.INT64_MAX, present[39], 2 ** 33])))
        # 1024 values: the 64 keys among 960 absent ones
        absent = [int(x) for x in rng.choice(2 ** 45, 960, replace=False)]
        absent = [v for v in absent if v not in set(present)][:960]
        out.append(("in", kf.IN, *csr([[present[:1], present[5:10], big_set(present, absent), [], [7, present[2], 2 ** 62]][i % 5]
                                        for i in range(nq)])))
    elif col == "distinct":
        out.append(("eq", kf.EQ, cyc([0, -3, 5, 10 ** 9, -1]), None))
        out.append(("range", kf.RANGE, cyc([-50, 0, 10, kf.INT64_MIN, -700]), cyc([50, 400, 9, kf.INT64_MAX, 700])))
        out.append(("in", kf.IN, *csr([[[-7], list(range(-10, 0, 2)), list(range(-512, 512)), [], [10 ** 9, 3]][i % 5] for i in range(nq)])))
    elif col == "skew":
        out.append(("eq", kf.EQ, cyc([2 ** 40, 3, 6, 4, 2 ** 40]), None))
        out.append(("range", kf.RANGE, cyc([0, 2 ** 40, kf.INT64_MIN, 100, 2 ** 41]), cyc([300, 2 ** 40, kf.INT64_MAX, 2 ** 41, 0])))
        out.append(("in", kf.IN, *csr([[[2 ** 40], [3, 6, 9, 12, 2 ** 40], list(range(3, 3 * 1024 + 3, 3)), [], [4, 5]][i % 5] for i in range(nq)])))
    else:
        raise KeyError(col)
    return out


class Case:
    """One shape's rows, queries, key columns and distance matrix; the references of partition calls over given indexed rows."""

    def __init__(self, name, nq=None):
        c = SHAPES[name]
        self.name, self.n, self.dim, self.kc, self.metric = name, c["n"], c["dim"], c["kc"], c["metric"]
        self.data, self.queries = draw(name, nq)
        self.nq = len(self.queries)
        self.columns = columns(self.n, 5000 + self.dim + 17)
        self.kind = "l2"
        self._d = None

    @property
    def d(self):
        if self._d is None:
            self._d = pr.distances(self.kind, self.metric, self.data, self.queries)
        return self._d

    def assert_distinct(self):
        for qi, row in enumerate(self.d):
            assert len(np.unique(pr.order_bits(self.kind, row))) == len(row), \
                f"shape {self.name}: two rows are equally far from query {qi} (seed {SHAPES[self.name]['qseeds'][qi]})"

    def filters(self, col):
        return filters(col, self.nq, 5000 + self.dim + 31)

    def partition(self, col, indexed=None):
        values, valid = self.columns[col]
        return pr.build(values, valid, np.arange(self.n) if indexed is None else indexed)

    def topk(self, part, flt, k, sqrt_out=False, allow=None):
        _, kind, a, b = flt
        return pr.topk_batch(part[0], part[1], kind, a, b, self.d, k, self.kind, sqrt_out, allow)


def tie_case():
    """Integer-valued rows (many equal distances) under a 4-valued key: (data, queries, keys int32)"""
    rng = np.random.default_rng(4)
    n, dim = 3000, 8
    return (rng.integers(0, 3, (n, dim)).astype(np.float32), rng.integers(0, 3, (5, dim)).astype(np.float32),
            rng.integers(0, 4, n).astype(np.int32))
