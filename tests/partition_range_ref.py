"""numpy restatement of the range search over a key partition (pqv.h: pqv_range_search_partition).

    sequence     partition_ref.sequence: query q's candidates, ordered by (key, row); n_candidates is its length, before the mask
    considered   the candidates the shared mask allows, at their UNMASKED positions
    hit          out <= radius on the OUTPUT scale (partition_ref.output: sqrt(d2) / d2, PQV_COSINE 0.5 d2, PQV_DOT 0 - s whatever
                 sqrt_out), inclusive; a NaN distance is never a hit
    order        ascending by (partition_ref.order_bits of the distance BEFORE the output transform, sequence position)
    max_results  > 0: the first max_results hits in that order; n_within counts all of them

Distances are partition_ref.distances' (the chains of range_oracle / cosine_ref / dot_ref)."""
import numpy as np

import partition_ref as pr


def range_query(prows, pkeys, kind, a, b, q, d_all, radius, dist_kind="l2", sqrt_out=False, allow=None, max_results=0):
    """-> (rows u32, dist f32, n_within, n_candidates, considered) of query q.  d_all: [n_rows] f32, partition_ref.distances()[q];
    allow: None or bools [n_rows], the shared mask."""
    seq = pr.sequence(pkeys, kind, a, b, q)
    cand = np.asarray(prows)[seq].astype(np.int64)
    pos = np.arange(len(cand))
    if allow is not None:
        keep = np.asarray(allow, bool)[cand]
        cand, pos = cand[keep], pos[keep]
    d = np.asarray(d_all, np.float32)[cand]
    out = np.asarray(pr.output(dist_kind, d, sqrt_out), np.float32)
    with np.errstate(invalid="ignore"):
        hit = np.nonzero(out <= np.float32(radius))[0]
    order = hit[np.lexsort((pos[hit], pr.order_bits(dist_kind, d[hit])))]
    n_within = len(order)
    if max_results:
        order = order[:max_results]
    return cand[order].astype(np.uint32), out[order], n_within, len(seq), len(cand)


def range_batch(prows, pkeys, kind, a, b, d, radius, dist_kind="l2", sqrt_out=False, allow=None, max_results=0):
    """-> (lims u64 [nq + 1], rows u32, dist f32, n_within u64 [nq], n_candidates u64 [nq], considered rows summed over the batch):
    pqv_range_search_partition's CSR form"""
    res = [range_query(prows, pkeys, kind, a, b, q, d[q], radius, dist_kind, sqrt_out, allow, max_results) for q in range(len(d))]
    lims = np.zeros(len(res) + 1, np.uint64)
    lims[1:] = np.cumsum([len(r[0]) for r in res])
    cat = lambda xs, t: np.concatenate(xs).astype(t) if xs else np.zeros(0, t)   # noqa: E731
    return (lims, cat([r[0] for r in res], np.uint32), cat([r[1] for r in res], np.float32), np.array([r[2] for r in res], np.uint64),
            np.array([r[3] for r in res], np.uint64), int(sum(r[4] for r in res)))


__all__ = ["range_query", "range_batch"]
