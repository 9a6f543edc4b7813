"""numpy restatement of the distinct / grouped top-k under a per-query key filter (pqv.h: pqv_topk_distinct_filtered,
pqv_topk_grouped_filtered): key_filter_ref's M_q -- filter validity AND F_q(filter key) AND the shared mask -- fed as the shared
mask to distinct_ref.distinct_topk / grouped_ref.grouped_topk, one query at a time.  The filter applies BEFORE a group's
representative is chosen."""
import numpy as np

import distinct_ref
import grouped_ref
import key_filter_ref
from range_oracle import REF4

EQ, RANGE, IN = key_filter_ref.EQ, key_filter_ref.RANGE, key_filter_ref.IN


def descriptor(kind, spec):
    """(kind, a, b) of pqv_key_filter from a test's spec: EQ a list of keys, RANGE a pair (lo, hi) of lists, IN a list of sets"""
    if kind == EQ:
        return EQ, np.asarray(spec, np.int64), None
    if kind == RANGE:
        return RANGE, np.asarray(spec[0], np.int64), np.asarray(spec[1], np.int64)
    lims, vals = key_filter_ref.sets_to_csr(spec)
    return IN, lims, vals


def call_kw(kind, spec):
    """the keywords Searcher.topk_distinct / topk_grouped take for the same spec"""
    if kind == EQ:
        return {"query_keys": np.asarray(spec, np.int64)}
    if kind == RANGE:
        return {"query_key_ranges": (np.asarray(spec[0], np.int64), np.asarray(spec[1], np.int64))}
    return {"query_key_sets": [list(s) for s in spec]}


def allowed(fvalues, fvalid, kind, spec, q, shared=None):
    """M_q as a bool array [n_rows]"""
    k, a, b = descriptor(kind, spec)
    return key_filter_ref.allowed_for(fvalues, fvalid, k, a, b, q, shared)


def distinct_topk(cand, group, gvalid, fvalues, fvalid, kind, spec, q, shared, data, query, k, metric=REF4, max_candidates=0):
    """-> distinct_ref.distinct_topk's (rows, d2, keys, n_candidates, n_considered) for query index q of the filter"""
    return distinct_ref.distinct_topk(cand, group, gvalid, allowed(fvalues, fvalid, kind, spec, q, shared), data, query, k, metric=metric,
                                      max_candidates=max_candidates)


def grouped_topk(cand, group, gvalid, fvalues, fvalid, kind, spec, q, shared, data, query, k, m, metric=REF4, max_candidates=0):
    """-> grouped_ref.grouped_topk's (rows [k, m], d2, keys [k], group_rows [k], n_found, n_candidates, n_considered)"""
    return grouped_ref.grouped_topk(cand, group, gvalid, allowed(fvalues, fvalid, kind, spec, q, shared), data, query, k, m, metric=metric,
                                    max_candidates=max_candidates)


def vacuity(cand, group, gvalid, fvalues, fvalid, kind, spec, q, shared, data, query, k, metric=REF4):
    """-> (a, b, c) of one query: (a) a returned group's representative differs from the one the call WITHOUT the filter picks for
    that group -- the group's nearest considered row fails F_q and another member passes, so filtering after the deduplication
    would be caught; (b) n_found < k; (c) n_found == k with groups cut off."""
    r, _, g, _, _ = distinct_topk(cand, group, gvalid, fvalues, fvalid, kind, spec, q, shared, data, query, k, metric)
    every, _, _, _, _ = distinct_topk(cand, group, gvalid, fvalues, fvalid, kind, spec, q, shared, data, query, len(cand) + 1, metric)
    ur, _, ug, _, _ = distinct_ref.distinct_topk(cand, group, gvalid, shared, data, query, len(cand) + 1, metric=metric)
    rep = dict(zip(ug.tolist(), ur.tolist()))
    a = any(rep[int(gg)] != int(rr) for rr, gg in zip(r, g))
    return a, len(r) < k, len(r) == k and len(every) > k
