"""numpy restatement of the grouped top-k (pqv.h: pqv_topk_grouped) over a candidate sequence.

The considered rows are distinct_ref's.  Sort them by (d2, position) -- the sequence S -- rank the key values by their first row in
S, keep the first k, and of each kept value its first m rows, in S order.  Distances are range_oracle.l2_chain's."""
import numpy as np

import distinct_ref
import mask_ref
from range_oracle import REF4, l2_chain

EMPTY = 0xFFFFFFFF


def group_sorted(rows, dist, column, k, m):
    """(rows, dist) already sorted by (d2, position) -> (rows [k, m] u32, dist [k, m] f32, keys [k] i64, group_rows [k] u32, n_found),
    padded as the call pads: 0xFFFFFFFF / +inf row slots, key 0 and count 0 group slots"""
    rows = np.asarray(rows, dtype=np.uint32)
    dist = np.asarray(dist, dtype=np.float32)
    keys = np.asarray(column)[rows.astype(np.int64)].astype(np.int64)
    o_r = np.full((k, m), EMPTY, np.uint32)
    o_d = np.full((k, m), np.inf, np.float32)
    o_g = np.zeros(k, np.int64)
    o_c = np.zeros(k, np.uint32)
    first = distinct_ref.first_per_key(keys, k)
    for g, f in enumerate(first):
        members = np.flatnonzero(keys == keys[f])[:m]            # ascending indices of S: S order
        o_r[g, :len(members)], o_d[g, :len(members)] = rows[members], dist[members]
        o_g[g], o_c[g] = keys[f], len(members)
    return o_r, o_d, o_g, o_c, len(first)


def grouped_topk(cand, column, valid, mask, data, query, k, m, metric=REF4, max_candidates=0):
    """-> (rows [k, m], d2 [k, m], keys [k], group_rows [k], n_found, n_candidates, n_considered)"""
    column = np.asarray(column)
    allowed = distinct_ref.considered_mask(len(column), valid, mask)
    rows, pos = mask_ref.considered(cand, allowed, max_candidates)
    d2 = l2_chain(np.asarray(data, dtype=np.float32)[rows].reshape(len(rows), -1), query, metric) if len(rows) else np.zeros(0, np.float32)
    order = np.lexsort((pos, d2))
    return group_sorted(rows[order], d2[order], column, k, m) + (len(cand), len(rows))
