"""numpy restatement of the per-query key filters (pqv.h: pqv_row_keys): the allow array M_q of one query, to be fed to
tests/mask_ref.py's considered / masked_topk / masked_range exactly as a caller's row mask is.

    M_q[r] = valid[r] && (int64) column[r] == key && (mask ? mask[r] : 1)

The comparison is made in i64: an int32 column is widened, the key never truncated -- so a key outside the i32 range matches
nothing on an int32 column -- and a NULL row (valid[r] == 0) never matches."""
import numpy as np

INT64_MIN, INT64_MAX = -(2 ** 63), 2 ** 63 - 1


def allowed_for(column, valid, key, mask=None):
    """-> bool [n_rows]: M_q.  column: int32 / int64 [n_rows]; valid: None or bytes / bools [n_rows] (0 = NULL); key: a Python or
    numpy integer within i64; mask: None or bools [n_rows]."""
    column = np.asarray(column)
    if column.dtype not in (np.int32, np.int64):
        raise TypeError(f"a key column is int32 or int64, got {column.dtype}")
    key = int(key)
    if not INT64_MIN <= key <= INT64_MAX:
        raise OverflowError("a query key is an int64")
    out = column.astype(np.int64) == np.int64(key)
    if valid is not None:
        out &= np.asarray(valid).astype(bool)
    if mask is not None:
        out &= np.asarray(mask).astype(bool)
    return out


def group_by_key(query_keys):
    """-> {key: [query indexes]} in first-appearance order: the calls of the route a keyed call replaces (one mask per distinct key)."""
    groups = {}
    for i, k in enumerate(query_keys):
        groups.setdefault(int(k), []).append(i)
    return groups
