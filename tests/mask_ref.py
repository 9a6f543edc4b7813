"""numpy restatement of the row-masked searches (pqv.h: pqv_topk_masked / pqv_range_search_masked) over a candidate sequence.

The candidate sequence is the unmasked call's (an oracle index' candidate_rows(q, nprobe); file-major on a table), cut by
max_candidates (or by per-file quotas, which the caller applies) BEFORE the mask is looked at; the considered rows are the
allowed ones among the capped candidates, at their unmasked positions; both searches order by (d2, position).  Distances are
range_oracle.l2_chain's: the reference's f32 chains, element by element."""
import numpy as np

from range_oracle import REF4, l2_chain


def considered(cand, allowed, max_candidates=0):
    """-> (rows, positions) of the considered candidates: capped first, then masked; positions are the unmasked ones."""
    cand = np.asarray(cand, dtype=np.uint32)
    if max_candidates:
        cand = cand[:max_candidates]
    keep = np.nonzero(np.asarray(allowed, dtype=bool)[cand])[0]
    return cand[keep], keep


def masked_topk(cand, allowed, data, query, k, metric=REF4, max_candidates=0):
    """-> (rows u32, d2 f32, n_candidates, n_considered): the k smallest considered candidates by (d2, position)."""
    rows, pos = considered(cand, allowed, max_candidates)
    d2 = l2_chain(np.asarray(data, dtype=np.float32)[rows].reshape(len(rows), -1), query, metric) if len(rows) else np.zeros(0, np.float32)
    order = np.lexsort((pos, d2))[:k]
    return rows[order], d2[order], len(cand), len(rows)


def masked_range(cand, allowed, data, query, radius, metric=REF4, sqrt_out=True, max_candidates=0, max_results=0, halve=False):
    """-> (rows u32, out f32, n_within, n_candidates): considered candidates with out <= radius by (d2, position); out = sqrt(d2),
    d2, or (halve: PQV_COSINE) 0.5 d2."""
    rows, pos = considered(cand, allowed, max_candidates)
    d2 = l2_chain(np.asarray(data, dtype=np.float32)[rows].reshape(len(rows), -1), query, metric) if len(rows) else np.zeros(0, np.float32)
    out = (np.float32(0.5) * d2) if halve else (np.sqrt(d2) if sqrt_out else d2)
    with np.errstate(invalid="ignore"):
        hit = np.nonzero(out <= np.float32(radius))[0]
    order = hit[np.lexsort((pos[hit], d2[hit]))]
    n_within = len(order)
    if max_results:
        order = order[:max_results]
    return rows[order], out[order].astype(np.float32), n_within, len(cand)


def filtered_lists(lists, allowed):
    """[list intersected with the allowed rows, in list order] -- the index of the filtered-lists setup."""
    allowed = np.asarray(allowed, dtype=bool)
    return [np.asarray(l, dtype=np.uint32)[allowed[np.asarray(l, dtype=np.int64)]] for l in lists]
