"""numpy restatement of the MMR contract (pqv.h: pqv_mmr_select, pqv_topk_mmr).

    candidates   one query has n candidates at positions 0 .. n-1 with rows r_i and rel_i, f32 on the call's output scale
    considered   the candidates whose row is indexed (rows_ref.considered: below the row count, not 0xFFFFFFFF, not removed) and
                 whose position is below n_found_in
    pd(a, b)     the metric's chain with row a in the query's place, on the output scale: pairwise_on_output_scale, the ONE place
                 where it is formed -- partition_ref.distances(kind, metric, data, data[rows]) through partition_ref.output
    red_t[i]     +0.0f while nothing is picked; then the running minimum of pd(r_s, r_i) over the picks, which starts at +inf with
                 the first pick and takes a value only where it compares smaller (a NaN never does)
    score_t[i]   (lambda * rel_i) - (om * red_t[i]), om = 1.0f - lambda: separate numpy float32 operations
    pick         the considered, not yet picked candidate with the smallest (dot_ref.ord_bits(score), position)
    outputs      in pick order: row, rel bit for bit, the score at the time of the pick; 0xFFFFFFFF / +inf / +inf behind them

The reference computes pd only for the rows it still needs (the live candidates'): every chain is row-wise, so a subset of the rows
gives the same bits as all of them."""
import numpy as np

from dot_ref import ord_bits
from partition_ref import distances, output
from rows_ref import considered

EMPTY = 0xFFFFFFFF


def pairwise_on_output_scale(kind, metric, data, rows, sqrt_out, against=None):
    """-> f32 [len(rows), len(against)]: pd(rows[s], against[i]) (against: row ids, None: every row of data)"""
    data = np.asarray(data, np.float32)
    others = data if against is None else data[np.asarray(against, np.int64)]
    if len(others) == 0:
        return np.zeros((len(rows), 0), np.float32)
    with np.errstate(all="ignore"):
        return output(kind, distances(kind, metric, others, data[np.asarray(rows, np.int64)]), sqrt_out)


class Pairwise:
    """pd over one case's rows: kind "l2" / "cos" / "dot", metric the chain's (REF4 / SEQ), sqrt_out the call's"""

    def __init__(self, kind, metric, data, sqrt_out):
        self.kind, self.metric, self.data, self.sqrt_out = kind, metric, np.asarray(data, np.float32), bool(sqrt_out)

    def __call__(self, row, against):
        return pairwise_on_output_scale(self.kind, self.metric, self.data, [row], self.sqrt_out, against)[0]


def select(cand, rel, k, lam, indexed, pd, n_found_in=None):
    """-> (rows u32 [k], dist f32 [k], score f32 [k], n_found) of one query.  cand: row ids [n]; rel: f32 [n]; indexed: bools
    [n_rows]; pd(row, against rows) -> f32 [len(against)]"""
    cand = np.asarray(cand, np.int64).reshape(-1)
    rel = np.ascontiguousarray(rel, np.float32).reshape(-1)
    n = len(cand)
    lim = n if n_found_in is None else min(n, int(n_found_in))
    live = considered(cand, indexed) & (np.arange(n) < lim)
    lam = np.float32(lam)
    om = np.float32(1.0) - lam
    red = np.zeros(n, np.float32)
    orow, od, osc = np.full(k, EMPTY, np.uint32), np.full(k, np.inf, np.float32), np.full(k, np.inf, np.float32)
    picks = 0
    while picks < k and live.any():
        with np.errstate(all="ignore"):
            a = lam * rel
            b = om * red
            score = (a - b).astype(np.float32)
        idx = np.nonzero(live)[0]
        j = idx[np.lexsort((idx, ord_bits(score[idx])))[0]]
        orow[picks], od[picks], osc[picks] = cand[j], rel[j], score[j]
        live[j] = False
        first = picks == 0
        picks += 1
        if picks == k or not live.any():
            break
        idx = np.nonzero(live)[0]
        p = np.asarray(pd(int(cand[j]), cand[idx]), np.float32)
        if first:
            red = np.full(n, np.inf, np.float32)
        red[idx] = np.where(p < red[idx], p, red[idx])
    return orow, od, osc, picks


def select_batch(cands, rels, k, lam, indexed, pd, n_found_in=None):
    """-> (rows [nq, k], dist [nq, k], score [nq, k], n_found u32 [nq]); cands / rels: [nq, n]"""
    res = [select(cands[q], rels[q], k, lam, indexed, pd, None if n_found_in is None else n_found_in[q]) for q in range(len(cands))]
    if not res:
        return np.zeros((0, k), np.uint32), np.zeros((0, k), np.float32), np.zeros((0, k), np.float32), np.zeros(0, np.uint32)
    return (np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.stack([r[2] for r in res]),
            np.array([r[3] for r in res], np.uint32))
