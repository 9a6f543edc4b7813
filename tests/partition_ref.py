"""numpy restatement of the key partition contract (pqv.h: pqv_key_partition, pqv_topk_partition).

    partition    the indexed rows (rows of some inverted list) whose key is valid, sorted by (key as i64, row id)
    sequence     query q's candidates: every partition row r with F_q(key[r]), ordered by (key[r], r) -- EQ and RANGE one
                 contiguous span of the partition, IN one span per slice value in the slice's ascending order; a candidate's
                 position is its index in the sequence; n_candidates is its length, before the mask
    considered   the candidates the shared mask allows, at their UNMASKED positions
    result       the k considered rows with the smallest (distance key, position), ascending

Distances are the chains the other restatements use: range_oracle.l2_chain (PQV_L2SQ_REF4 / PQV_L2SQ_SEQ), cosine_ref over it
(PQV_COSINE: the chain of the normalised vectors, halved), dot_ref.dist (PQV_DOT: 0 - s, ordered by ord_bits).  The distance key of
the L2 forms is the f32 bit pattern of d2 (non-negative: bit order is value order)."""
import numpy as np

import cosine_ref
import dot_ref
from key_filter_ref import EQ, IN, RANGE, INT64_MAX, INT64_MIN
from range_oracle import REF4, SEQ, l2_chain

EMPTY = 0xFFFFFFFF
KINDS = ("l2", "cos", "dot")


def build(values, valid, indexed_rows):
    """-> (rows u32 [m], keys i64 [m]): the partition of a key column (int32 / int64 [n_rows], valid: None or bytes [n_rows]) over
    the indexed rows, in (key, row) order."""
    values = np.asarray(values)
    if values.dtype not in (np.int32, np.int64):
        raise TypeError(f"a key column is int32 or int64, got {values.dtype}")
    rows = np.unique(np.asarray(indexed_rows, dtype=np.int64))
    if valid is not None:
        rows = rows[np.asarray(valid)[rows] != 0]
    keys = values[rows].astype(np.int64)
    order = np.lexsort((rows, keys))
    return rows[order].astype(np.uint32), keys[order]


def distinct(pkeys):
    """-> (values i64 ascending, counts u64) of a partition's keys"""
    v, c = np.unique(np.asarray(pkeys, dtype=np.int64), return_counts=True)
    return v.astype(np.int64), c.astype(np.uint64)


def _span(pkeys, lo, hi):
    if lo > hi:
        return 0, 0
    return int(np.searchsorted(pkeys, lo, side="left")), int(np.searchsorted(pkeys, hi, side="right"))


def sequence(pkeys, kind, a, b, q):
    """-> indices into the partition (int64), in sequence order, of query q's candidates"""
    pkeys = np.asarray(pkeys, dtype=np.int64)

    def i64(v):
        v = int(v)
        if not INT64_MIN <= v <= INT64_MAX:
            raise OverflowError("a query key is an int64")
        return v

    if kind == EQ:
        s0, s1 = _span(pkeys, i64(a[q]), i64(a[q]))
        return np.arange(s0, s1, dtype=np.int64)
    if kind == RANGE:
        s0, s1 = _span(pkeys, i64(a[q]), i64(b[q]))
        return np.arange(s0, s1, dtype=np.int64)
    if kind == IN:
        l0, l1 = int(a[q]), int(a[q + 1])
        vals = [i64(v) for v in b[l0:l1]]
        assert all(x < y for x, y in zip(vals, vals[1:])), "query key sets must be strictly ascending"
        parts = [np.arange(*_span(pkeys, v, v), dtype=np.int64) for v in vals]
        return np.concatenate(parts) if parts else np.zeros(0, np.int64)
    raise ValueError(f"unknown key filter kind {kind}")


def distances(kind, metric, data, queries):
    """[nq, n] f32: every row's distance to every query BEFORE the output transform -- d2; PQV_COSINE: d2 of the normalised
    vectors; PQV_DOT: 0 - s"""
    data, queries = np.asarray(data, np.float32), np.asarray(queries, np.float32)
    if kind == "dot":
        return np.stack([dot_ref.dist(q, data) for q in queries])
    if kind == "cos":
        data, queries = cosine_ref.normalise(data), cosine_ref.normalise(queries)
    return np.stack([l2_chain(data, q, metric) for q in queries])


def order_bits(kind, d):
    """u32 whose ascending order is the device key's: ord(dist) for PQV_DOT, the f32 bits of d2 otherwise"""
    d = np.ascontiguousarray(d, dtype=np.float32)
    return dot_ref.ord_bits(d) if kind == "dot" else d.view(np.uint32)


def output(kind, d, sqrt_out):
    if kind == "cos":
        return cosine_ref.half(d)
    if kind == "l2" and sqrt_out:
        return np.sqrt(d).astype(np.float32)
    return np.asarray(d, np.float32)


def topk(prows, pkeys, kind, a, b, q, d_all, k, dist_kind="l2", sqrt_out=False, allow=None):
    """-> (rows u32 [k], dist f32 [k], n_found, n_candidates) of query q.  d_all: [n_rows] f32, distances()[q]; allow: None or
    bools [n_rows], the shared mask."""
    seq = sequence(pkeys, kind, a, b, q)
    cand = np.asarray(prows)[seq].astype(np.int64)
    pos = np.arange(len(cand))
    if allow is not None:
        keep = np.asarray(allow, bool)[cand]
        cand, pos = cand[keep], pos[keep]
    d = np.asarray(d_all, np.float32)[cand]
    order = np.lexsort((pos, order_bits(dist_kind, d)))[:k]
    orow, od = np.full(k, EMPTY, np.uint32), np.full(k, np.inf, np.float32)
    orow[:len(order)] = cand[order]
    od[:len(order)] = output(dist_kind, d[order], sqrt_out)
    return orow, od, len(order), len(seq), len(cand)


def topk_batch(prows, pkeys, kind, a, b, d, k, dist_kind="l2", sqrt_out=False, allow=None):
    """-> (rows [nq, k], dist [nq, k], n_found u32 [nq], n_candidates u64 [nq], considered rows summed over the batch)"""
    res = [topk(prows, pkeys, kind, a, b, q, d[q], k, dist_kind, sqrt_out, allow) for q in range(len(d))]
    return (np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.array([r[2] for r in res], np.uint32),
            np.array([r[3] for r in res], np.uint64), int(sum(r[4] for r in res)))


__all__ = ["EQ", "RANGE", "IN", "REF4", "SEQ", "build", "distinct", "sequence", "distances", "order_bits", "output", "topk", "topk_batch"]
