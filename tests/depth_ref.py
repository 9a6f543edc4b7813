"""Numpy restatement of the per-query probe depth rule (pqv.h: pqv_topk_depth), over the ORACLE.

With kc lists, p0 = min(nprobe, kc) and P = min(max_nprobe, kc), the probe order c_0 .. c_{P-1} is the oracle's
find_closest_centroids(q, P) and d2_j = oracle.l2_ref4(q, centroid c_j).  The raw depth r is the caller's (GIVEN), or the number
of j < P with d2_j <= t, t the ONE float32 product d2_ratio * d2_0 (RATIO; a NaN on either side compares false).  The depth used
is min(max(r, p0), P).  PQV_COSINE: the same rule over the normalised centroids and the normalised queries (tests/cosine_ref.py).
Nothing here looks at the code under test."""
import numpy as np


def probe_order(oracle_index, q, max_nprobe):
    return np.asarray(oracle_index.find_closest_centroids(q, max_nprobe)).astype(np.int64)


def probe_d2(oracle, oracle_index, q, max_nprobe):
    """float32 [P]: the probe distances of q's probe order"""
    q = np.ascontiguousarray(q, dtype=np.float32)
    cents = np.asarray(oracle_index.centroids, np.float32).reshape(-1, len(q))
    return np.array([oracle.l2_ref4(q, cents[c]) for c in probe_order(oracle_index, q, max_nprobe)], dtype=np.float32)


def ratio_count(d2, d2_ratio):
    """the raw RATIO depth of one query from its probe distances: threshold product and comparison in float32"""
    d2 = np.asarray(d2, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.float32(d2_ratio) * d2[0]
        assert t.dtype == np.float32
        return int(np.count_nonzero(d2 <= t))      # (NaN <= x and x <= NaN are False)


def clamp(raw, nprobe, max_nprobe, kc):
    if max_nprobe < nprobe:
        raise ValueError("max_nprobe must be >= nprobe")
    p0, P = min(nprobe, kc), min(max_nprobe, kc)
    return min(max(int(raw), p0), P)


def used_given(depths, nprobe, max_nprobe, kc):
    return np.array([clamp(r, nprobe, max_nprobe, kc) for r in depths], np.uint32)


def used_ratio(oracle, oracle_index, queries, d2_ratio, nprobe, max_nprobe):
    kc = int(oracle_index.n_clusters)
    P = min(max_nprobe, kc)
    return np.array([clamp(ratio_count(probe_d2(oracle, oracle_index, q, P), d2_ratio), nprobe, max_nprobe, kc) for q in queries], np.uint32)


def cosine_index_and_queries(oracle, oracle_index, lists, queries):
    """the index and the queries the PQV_COSINE probe ranks: both normalised"""
    from cosine_ref import normalise
    dim = np.asarray(queries).shape[-1]
    n_oidx = oracle.index_from_parts(dim, normalise(np.asarray(oracle_index.centroids, np.float32).reshape(-1, dim)), lists)
    return n_oidx, normalise(queries)
