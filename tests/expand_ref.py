"""Numpy restatement of the expanding filtered top-k's depth rule (pqv.h: pqv_topk_expand), over the ORACLE's probe order.

With kc lists, p0 = min(nprobe, kc) and P = min(max_nprobe, kc), cnt(p) = the rows of M_q in the first p lists of
find_closest_centroids(q, P): nprobe_used = the smallest p in [p0, P] with cnt(p) >= k, or P if there is none.  A row counts
whatever its distance is.  Nothing here looks at the code under test."""
import numpy as np


def probe_order(oracle_index, q, max_nprobe):
    """The first min(max_nprobe, kc) lists of q's probe order (stable by (d2, id): the nearest P begin with the nearest p)."""
    return np.asarray(oracle_index.find_closest_centroids(q, max_nprobe)).astype(np.int64)


def prefix_counts(oracle_index, lists, M_q, q, max_nprobe):
    """cnt(1 .. P) as int64"""
    M_q = np.asarray(M_q, bool)
    order = probe_order(oracle_index, q, max_nprobe)
    per = [int(M_q[np.asarray(lists[c]).astype(np.int64)].sum()) for c in order]
    return np.cumsum(np.array(per, np.int64))


def nprobe_used(oracle_index, lists, M_q, q, k, nprobe, max_nprobe):
    kc = len(lists)
    if max_nprobe < nprobe:
        raise ValueError("max_nprobe must be >= nprobe")
    p0, P = min(nprobe, kc), min(max_nprobe, kc)
    cnt = prefix_counts(oracle_index, lists, M_q, q, P)
    assert len(cnt) == P
    for p in range(p0, P + 1):
        if cnt[p - 1] >= k:
            return p
    return P


def n_candidates(oracle_index, lists, q, used):
    """the summed length of the first `used` lists of q's probe order"""
    return int(sum(len(lists[c]) for c in probe_order(oracle_index, q, used)))


def used_for_batch(oracle_index, lists, masks, queries, k, nprobe, max_nprobe):
    """masks: one M for the batch (1-D) or one per query (2-D / a list)"""
    masks = np.asarray(masks)
    per_query = masks.ndim == 2
    return np.array([nprobe_used(oracle_index, lists, masks[i] if per_query else masks, q, k, nprobe, max_nprobe)
                     for i, q in enumerate(queries)], np.uint32)
