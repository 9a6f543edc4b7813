"""Numpy restatement of the expanding distinct / grouped top-k's depth rule (pqv.h: pqv_topk_distinct_expand), over the ORACLE's
probe order, and a host model of the counting kernel's hash set.

With kc lists, p0 = min(nprobe, kc) and P = min(max_nprobe, kc), gcnt(p) = the DISTINCT i64 group values among the rows r of the
first p lists of find_closest_centroids(q, P) with group_valid[r] and M_q[r]: nprobe_used = the smallest p in [p0, P] with
gcnt(p) >= k, or P if there is none.  A row counts whatever its distance is; group_size plays no part.  M_q comes from
distinct_filter_ref.allowed (filter validity AND F_q AND the shared mask) or is the shared mask itself.  Nothing here looks at the
code under test."""
import numpy as np

import expand_ref

# the set of group_expand_kernel (csrc/kernels.h): capacity, empty marker, home slot, linear probing
SET_SLOTS = 4096
SET_EMPTY = 2 ** 64 - 1          # the bits of the group value -1: counted by a flag of its own, never stored
_M64 = 2 ** 64 - 1


def set_home(v):
    return (((v & _M64) * 0x9E3779B97F4A7C15) & _M64) >> 52


class GroupSet:
    """The kernel's set, one insert at a time: -> True iff the value was new.  `steps` counts the slots looked at."""

    def __init__(self):
        self.tab = [SET_EMPTY] * SET_SLOTS
        self.marker = False
        self.count = 0
        self.steps = 0

    def insert(self, value):
        v = int(value) & _M64
        if v == SET_EMPTY:
            new = not self.marker
            self.marker = True
            self.count += new
            return new
        h = set_home(v)
        for i in range(SET_SLOTS):
            at = (h + i) % SET_SLOTS
            self.steps += 1
            if self.tab[at] == SET_EMPTY:
                self.tab[at] = v
                self.count += 1
                return True
            if self.tab[at] == v:
                return False
        return False


def _allowed(group_valid, M_q, n):
    ok = np.ones(n, bool) if group_valid is None else np.asarray(group_valid).astype(bool)
    return ok if M_q is None else ok & np.asarray(M_q).astype(bool)


def gcnt(oracle_index, lists, group, group_valid, M_q, q, max_nprobe):
    """gcnt(1 .. P) as int64"""
    group = np.asarray(group).astype(np.int64)
    ok = _allowed(group_valid, M_q, len(group))
    seen, out = set(), []
    for c in expand_ref.probe_order(oracle_index, q, max_nprobe):
        rows = np.asarray(lists[c]).astype(np.int64)
        seen.update(group[rows[ok[rows]]].tolist())
        out.append(len(seen))
    return np.array(out, np.int64)


def nprobe_used(oracle_index, lists, group, group_valid, M_q, q, k, nprobe, max_nprobe):
    kc = len(lists)
    if max_nprobe < nprobe:
        raise ValueError("max_nprobe must be >= nprobe")
    p0, P = min(nprobe, kc), min(max_nprobe, kc)
    cnt = gcnt(oracle_index, lists, group, group_valid, M_q, q, P)
    assert len(cnt) == P
    for p in range(p0, P + 1):
        if cnt[p - 1] >= k:
            return p
    return P


def row_depth(oracle_index, lists, group_valid, M_q, q, k, nprobe, max_nprobe):
    """the row-counting depth (expand_ref.nprobe_used) of the same row set"""
    n = int(max(int(np.max(l)) for l in lists if len(l))) + 1
    return expand_ref.nprobe_used(oracle_index, lists, _allowed(group_valid, M_q, n), q, k, nprobe, max_nprobe)


def used_for_batch(oracle_index, lists, group, group_valid, masks, queries, k, nprobe, max_nprobe):
    """masks: None, one M for the batch (1-D) or one per query (2-D / a list)"""
    per_query = masks is not None and np.asarray(masks).ndim == 2
    return np.array([nprobe_used(oracle_index, lists, group, group_valid, (masks[i] if per_query else masks), q, k, nprobe, max_nprobe)
                     for i, q in enumerate(queries)], np.uint32)
