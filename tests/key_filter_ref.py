"""numpy restatement of the per-query filter descriptor (pqv.h: pqv_key_filter): the allow array M_q of one query, to be fed to
tests/mask_ref.py's considered / masked_topk / masked_range -- or to Searcher.row_mask -- exactly as a caller's row mask is.

    M_q[r] = valid[r] && F_q((int64) column[r]) && (mask ? mask[r] : 1)

    EQ     F_q(v) = v == a[q]
    RANGE  F_q(v) = a[q] <= v && v <= b[q]            (both ends inclusive; a[q] > b[q]: nothing)
    IN     F_q(v) = v is one of b[a[q] .. a[q + 1])   (a: offsets [nq + 1]; an empty slice: nothing)

Every comparison is made in i64: an int32 column is widened, a bound or a set value never truncated, and a NULL row
(valid[r] == 0) never matches."""
import numpy as np

EQ, RANGE, IN = 0, 1, 2
SET_MAX = 1024
INT64_MIN, INT64_MAX = -(2 ** 63), 2 ** 63 - 1


def _i64(v):
    v = int(v)
    if not INT64_MIN <= v <= INT64_MAX:
        raise OverflowError("a query key is an int64")
    return np.int64(v)


def allowed_for(values, valid, kind, a, b, q, shared=None):
    """-> bool [n_rows]: M_q.  values: int32 / int64 [n_rows]; valid: None or bytes / bools [n_rows] (0 = NULL); kind, a, b: the
    descriptor's, as sequences of Python or numpy integers; q: the query; shared: None or bools [n_rows], the call's mask."""
    values = np.asarray(values)
    if values.dtype not in (np.int32, np.int64):
        raise TypeError(f"a key column is int32 or int64, got {values.dtype}")
    wide = values.astype(np.int64)
    if kind == EQ:
        out = wide == _i64(a[q])
    elif kind == RANGE:
        out = (wide >= _i64(a[q])) & (wide <= _i64(b[q]))
    elif kind == IN:
        s0, s1 = int(a[q]), int(a[q + 1])
        if s1 < s0:
            raise ValueError("query key sets must start at 0 and not decrease")
        members = np.array([_i64(v) for v in b[s0:s1]], dtype=np.int64)
        out = np.isin(wide, members)
    else:
        raise ValueError(f"unknown key filter kind {kind}")
    if valid is not None:
        out &= np.asarray(valid).astype(bool)
    if shared is not None:
        out &= np.asarray(shared).astype(bool)
    return out


def sets_to_csr(sets):
    """-> (lims uint64 [nq + 1], vals int64): every set sorted with duplicates removed, the form PQV_KEY_IN takes."""
    lims, vals = [0], []
    for s in sets:
        u = sorted({int(_i64(v)) for v in s})
        if len(u) > SET_MAX:
            raise ValueError(f"a query key set takes at most {SET_MAX} values")
        vals += u
        lims.append(len(vals))
    return np.array(lims, np.uint64), np.array(vals, np.int64)
