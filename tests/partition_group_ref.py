"""numpy restatement of the distinct / grouped top-k over a key partition (pqv.h: pqv_topk_partition_grouped).

    candidates   partition_ref.sequence: pqv_topk_partition's sequence for the query's filter; a candidate's position is its index
                 in it; n_candidates is its length, before the mask and the group validity
    considered   the candidates the shared mask allows AND whose group value is valid, at their unmasked positions
    result       S = the considered rows sorted by (distance key, position); grouped_ref.group_sorted over S: groups compared in
                 i64 and ranked by their first row in S, the first k kept, each with its first min(m, rows it has) rows in S order

Distances are partition_ref.distances'.  Beside the outputs a query reports the considered rows (what pass 1 evaluates) and the
considered rows of the selected groups (what pass 2 evaluates when m > 1)."""
import numpy as np

import grouped_ref
import partition_ref as pr

EMPTY = 0xFFFFFFFF


def grouped(prows, pkeys, kind, a, b, q, d_all, group_values, group_valid, k, m, dist_kind="l2", sqrt_out=False, allow=None):
    """-> (rows u32 [k, m], dist f32 [k, m], group_key i64 [k], group_rows u32 [k], n_found, n_candidates, considered, pass 2 rows)
    of query q.  d_all: [n_rows] f32, distances()[q]; group_values: int32 / int64 [n_rows]; group_valid: None or bytes [n_rows];
    allow: None or bools [n_rows], the shared mask."""
    seq = pr.sequence(pkeys, kind, a, b, q)
    cand = np.asarray(prows)[seq].astype(np.int64)
    pos = np.arange(len(cand))
    keep = np.ones(len(cand), bool)
    if allow is not None:
        keep &= np.asarray(allow, bool)[cand]
    if group_valid is not None:
        keep &= np.asarray(group_valid)[cand] != 0
    cand, pos = cand[keep], pos[keep]
    d = np.asarray(d_all, np.float32)[cand]
    order = np.lexsort((pos, pr.order_bits(dist_kind, d)))
    s_rows, s_d = cand[order], d[order]
    o_r, o_d, o_g, o_c, nf = grouped_ref.group_sorted(s_rows, pr.output(dist_kind, s_d, sqrt_out), group_values, k, m)
    in_selected = np.isin(np.asarray(group_values)[cand].astype(np.int64), o_g[:nf])
    return o_r, o_d, o_g, o_c, nf, len(seq), len(cand), int(in_selected.sum())


def grouped_batch(prows, pkeys, kind, a, b, d, group_values, group_valid, k, m, dist_kind="l2", sqrt_out=False, allow=None):
    """-> (rows [nq, k, m], dist [nq, k, m], group_key [nq, k], group_rows [nq, k], n_found u32 [nq], n_candidates u64 [nq],
    considered rows summed over the batch, pass 2 rows summed over the batch)"""
    res = [grouped(prows, pkeys, kind, a, b, q, d[q], group_values, group_valid, k, m, dist_kind, sqrt_out, allow) for q in range(len(d))]
    return (np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.stack([r[2] for r in res]), np.stack([r[3] for r in res]),
            np.array([r[4] for r in res], np.uint32), np.array([r[5] for r in res], np.uint64), int(sum(r[6] for r in res)),
            int(sum(r[7] for r in res)))


__all__ = ["grouped", "grouped_batch"]
