"""numpy model of pqv_index_append (test infrastructure): the splice rule and the row-bound rule, with the assignment taken from
tests/assign_exact.py -- none of it is code under test.

Splice rule: list c of the result = list c of the old index, verbatim, followed by first_row + (the rows of the range assigned
to c, ascending).  When the old lists are themselves the nearest-centroid lists of rows [0, n0) and the range is [n0, n0 + m), that
is what the reference's final loop (src/ivf/index.rs:189-206) leaves for these centroids over all n0 + m rows.
Row-bound rule: bound = largest indexed row id + 1 (0 for empty lists); an append must start at or above it, and leaves
first_row + n_rows behind."""
import numpy as np

import assign_exact


def row_bound(lists):
    return max((int(l.max()) + 1 for l in lists if len(l)), default=0)


def splice(old_lists, assign_new, first_row):
    """old_lists: k arrays of row ids; assign_new [m]: cluster of row first_row + i.  -> k uint32 arrays."""
    assign_new = np.asarray(assign_new)
    out = []
    for c, old in enumerate(old_lists):
        new = (np.nonzero(assign_new == c)[0] + first_row).astype(np.uint32)       # ascending
        out.append(np.concatenate([np.asarray(old, np.uint32), new]))
    return out


def append_lists(old_lists, X_all, C, first_row, n_rows):
    """-> (lists after appending rows [first_row, first_row + n_rows) of X_all, their assignment).  Raises ValueError where
    pqv_index_append refuses the range."""
    if first_row + n_rows > len(X_all):
        raise ValueError("range past the corpus")
    if first_row < row_bound(old_lists):
        raise ValueError("first_row below the row bound")
    if n_rows == 0:
        return [np.asarray(l, np.uint32) for l in old_lists], np.zeros(0, np.uint32)
    assign = assign_exact.nearest(X_all[first_row:first_row + n_rows], C)[0]
    return splice(old_lists, assign, first_row), assign


def blob(oracle, dim, C, lists):
    return oracle.index_from_parts(dim, C, lists).to_bytes()


def offsets_and_rows(lists):
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint64)
    rows = np.concatenate(lists).astype(np.uint32) if len(lists) else np.zeros(0, np.uint32)
    return off, rows
