"""numpy restatement of the candidate-list contract (pqv.h: pqv_topk_rows, pqv_score_rows).

    sequence     query q's candidates: cand_rows[lims[q] : lims[q + 1]] exactly as given -- any order, duplicates kept; a candidate's
                 position is its index in the slice; n_candidates is the slice's length, before any test
    considered   the candidates whose row is indexed (a row of some inverted list: below the row count, not 0xFFFFFFFF, not removed)
                 and which the shared mask allows, at their UNMASKED positions
    top-k        the k considered candidates with the smallest (distance key, position), ascending; 0xFFFFFFFF / +inf behind them
    scores       per candidate its distance on the output scale, +inf where it is not considered

Distances are the chains the other restatements use, through partition_ref: range_oracle.l2_chain (PQV_L2SQ_REF4 / PQV_L2SQ_SEQ),
cosine_ref over it (PQV_COSINE: the chain of the normalised vectors, halved), dot_ref.dist (PQV_DOT: 0 - s, ordered by ord_bits)."""
import numpy as np

from partition_ref import distances, order_bits, output

EMPTY = 0xFFFFFFFF


def csr(lists, base=0):
    """-> (lims u64 [nq + 1] starting at `base`, rows u32 with `base` unread ids in front) of per-query lists"""
    lists = [np.asarray(l, dtype=np.uint32).reshape(-1) for l in lists]
    lims = np.zeros(len(lists) + 1, np.uint64)
    lims[1:] = np.cumsum([len(l) for l in lists])
    rows = np.concatenate([np.full(base, 0xDEADBEEF, np.uint32)] + lists) if lists or base else np.zeros(0, np.uint32)
    return lims + np.uint64(base), rows.astype(np.uint32)


def considered(cand, indexed, allow=None):
    """-> bools [len(cand)]: which candidates are considered.  indexed: bools [n_rows]; allow: None or bools [n_rows]"""
    cand = np.asarray(cand, dtype=np.int64)
    indexed = np.asarray(indexed, bool)
    ok = cand < len(indexed)                        # (0xFFFFFFFF is at or above every row count)
    at = np.where(ok, cand, 0)
    ok &= indexed[at]
    if allow is not None:
        ok &= np.asarray(allow, bool)[at]
    return ok


def scores(cand, indexed, d_all, dist_kind="l2", sqrt_out=False, allow=None):
    """-> f32 [len(cand)]: every candidate's distance on the output scale, +inf where it is not considered.  d_all: [n_rows] f32,
    partition_ref.distances()[q]"""
    cand = np.asarray(cand, dtype=np.int64)
    ok = considered(cand, indexed, allow)
    out = np.full(len(cand), np.inf, np.float32)
    out[ok] = output(dist_kind, np.asarray(d_all, np.float32)[cand[ok]], sqrt_out)
    return out


def topk(cand, indexed, d_all, k, dist_kind="l2", sqrt_out=False, allow=None):
    """-> (rows u32 [k], dist f32 [k], n_found, n_candidates, n_considered) of one query"""
    cand = np.asarray(cand, dtype=np.int64)
    pos = np.nonzero(considered(cand, indexed, allow))[0]
    rows = cand[pos]
    d = np.asarray(d_all, np.float32)[rows]
    order = np.lexsort((pos, order_bits(dist_kind, d)))[:k]
    orow, od = np.full(k, EMPTY, np.uint32), np.full(k, np.inf, np.float32)
    orow[:len(order)] = rows[order]
    od[:len(order)] = output(dist_kind, d[order], sqrt_out)
    return orow, od, len(order), len(cand), len(rows)


def topk_batch(lists, indexed, d, k, dist_kind="l2", sqrt_out=False, allow=None):
    """-> (rows [nq, k], dist [nq, k], n_found u32 [nq], n_candidates u64 [nq], considered candidates summed over the batch)"""
    res = [topk(lists[q], indexed, d[q], k, dist_kind, sqrt_out, allow) for q in range(len(lists))]
    return (np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.array([r[2] for r in res], np.uint32),
            np.array([r[3] for r in res], np.uint64), int(sum(r[4] for r in res)))


def scores_batch(lists, indexed, d, dist_kind="l2", sqrt_out=False, allow=None):
    """-> (lims u64 [nq + 1] from 0, dist f32 [lims[nq]])"""
    parts = [scores(lists[q], indexed, d[q], dist_kind, sqrt_out, allow) for q in range(len(lists))]
    lims = np.zeros(len(lists) + 1, np.uint64)
    lims[1:] = np.cumsum([len(p) for p in parts])
    return lims, (np.concatenate(parts) if parts else np.zeros(0, np.float32)).astype(np.float32)


def topk_from_scores(cand, sc, k, dist_kind="l2"):
    """-> (rows u32 [k], dist f32 [k], n_found): the top-k of one query from a score call's answer `sc` for it, taken with sqrt_out
    = False (the output scale then keeps the key's order: d2 itself, 0 - s, or -- PQV_COSINE -- the exact halving): the stable sort
    of the finite-or-NaN scores by (order bits, position).  +inf marks a candidate that is not considered."""
    cand = np.asarray(cand, dtype=np.int64)
    sc = np.asarray(sc, np.float32)
    pos = np.nonzero(~np.isposinf(sc))[0]
    order = pos[np.lexsort((pos, order_bits("dot" if dist_kind == "dot" else "l2", sc[pos])))][:k]
    orow, od = np.full(k, EMPTY, np.uint32), np.full(k, np.inf, np.float32)
    orow[:len(order)] = cand[order]
    od[:len(order)] = sc[order]
    return orow, od, len(order)


__all__ = ["EMPTY", "csr", "considered", "scores", "topk", "topk_batch", "scores_batch", "topk_from_scores", "distances", "order_bits", "output"]
