"""numpy restatement of the distinct top-k (pqv.h: pqv_topk_distinct) over a candidate sequence.

The considered rows are mask_ref.considered's -- the unmasked candidate sequence cut by max_candidates first, then the rows whose
key is valid and which the mask allows, at their unmasked positions.  Sort them by (d2, position), keep the first row of every key
value (compared in i64), cut to k.  Distances are range_oracle.l2_chain's."""
import numpy as np

import mask_ref
from range_oracle import REF4, l2_chain


def considered_mask(n_rows, valid=None, mask=None):
    """the allow array of a distinct call: key validity AND the shared mask"""
    a = np.ones(n_rows, dtype=bool)
    if valid is not None:
        a &= np.asarray(valid).astype(bool)
    if mask is not None:
        a &= np.asarray(mask).astype(bool)
    return a


def first_per_key(keys, k):
    """indices of the first occurrence of every value of keys (i64), in order, at most k of them"""
    keys = np.asarray(keys, dtype=np.int64)
    if len(keys) == 0:
        return np.zeros(0, dtype=np.int64)
    _, first = np.unique(keys, return_index=True)
    return np.sort(first)[:k]


def dedup_sorted(rows, dist, column, k):
    """(rows, dist) already sorted by (d2, position) -> (rows, dist, keys) of the first row per key value, cut to k"""
    rows = np.asarray(rows, dtype=np.uint32)
    keys = np.asarray(column)[rows.astype(np.int64)].astype(np.int64)
    keep = first_per_key(keys, k)
    return rows[keep], np.asarray(dist, dtype=np.float32)[keep], keys[keep]


def distinct_topk(cand, column, valid, mask, data, query, k, metric=REF4, max_candidates=0):
    """-> (rows u32, d2 f32, keys i64, n_candidates, n_considered)"""
    column = np.asarray(column)
    allowed = considered_mask(len(column), valid, mask)
    rows, pos = mask_ref.considered(cand, allowed, max_candidates)
    d2 = l2_chain(np.asarray(data, dtype=np.float32)[rows].reshape(len(rows), -1), query, metric) if len(rows) else np.zeros(0, np.float32)
    order = np.lexsort((pos, d2))
    r, d, g = dedup_sorted(rows[order], d2[order], column, k)
    return r, d, g, len(cand), len(rows)
