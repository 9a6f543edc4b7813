"""The inputs of the filtered distinct / grouped tests (tests/test_gpu_distinct_filter.py on the GPU,
tests/test_distinct_filter_host.py without one): the key columns and the per-query filters, drawn from committed seeds.

A shape of test_gpu_mask.SHAPES gets a tenant column (the filter column: N_TENANTS values) and a doc column (the group column:
about 16 rows per doc, docs spanning tenants), both drawn from SEEDS[shape] -- independent of the rows and queries, which
test_gpu_mask.Setup draws from seed 11 + dim.  The seeds were searched on the CPU (the first of 1, 2, ... that meets
test_distinct_filter_host.py's non-vacuity conditions for every filter kind); nothing here needs a GPU."""
import numpy as np

from distinct_filter_ref import EQ, IN, RANGE

N_TENANTS = 8
NQ = 5                      # test_gpu_mask.Setup draws 5 queries
KS = (1, 5, 64, 65, 200)
KINDS = {"eq": EQ, "range": RANGE, "in": IN}
# shape -> the seed of its columns
SEEDS = {"4096x128": 1, "2048x256": 1, "1500x30": 1, "2048x32-seq": 1}

# one filter per kind over the tenant values 0 .. 7, NQ queries each
SPECS = {
    "eq": [3, 0, 7, 5, 2],
    "range": ([0, 2, 6, 3, 5], [1, 2, 7, 7, 4]),                      # the last query's is empty (lo > hi)
    "in": [[0, 5], [1], [2, 3, 4, 6], [7, 11], []],                   # 11 is no tenant; the last query's set is empty
}


def columns(shape, n, fdtype=np.int32, gdtype=np.int32):
    """-> (tenant [n] fdtype, doc [n] gdtype)"""
    rng = np.random.default_rng(SEEDS[shape])
    tenant = rng.integers(0, N_TENANTS, n)
    doc = rng.integers(0, n // 16, n)
    return tenant.astype(fdtype), doc.astype(gdtype)
