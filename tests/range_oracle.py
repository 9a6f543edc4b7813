"""numpy restatement of range search over an oracle-built index (the answer pqv_range_search must give, bit for bit).

Candidates come from the C oracle's candidate_rows (probe-rank order, list order inside a list); distances follow the
reference's f32 chains element by element -- PQV_L2SQ_REF4 (src/ivf/index.rs:461-480): per group of four
t = ((d0^2 + d1^2) + d2^2) + d3^2, sum += t, then the scalar tail; PQV_L2SQ_SEQ (src/df_vector/exec.rs:529-533):
sum += d^2 element by element.  numpy rounds every f32 operation on its own (no fused multiply-add), so the bits equal the
C oracle's pqo_squared_l2_ref4 / pqo_squared_l2_seq (tests/test_range_host.py checks that)."""
import numpy as np

REF4, SEQ = 0, 1


def l2_chain(rows, query, metric):
    """d2 [m] f32 of rows [m, dim] against query [dim] (or row by row against queries [m, dim]) in the metric's
    summation order."""
    x = np.ascontiguousarray(rows, dtype=np.float32)
    q = np.ascontiguousarray(query, dtype=np.float32)
    m, dim = x.shape
    d = (q.reshape(1, -1) if q.ndim < 2 else q) - x
    sq = d * d
    s = np.zeros(m, dtype=np.float32)
    if metric == SEQ:
        for e in range(dim):
            s = s + sq[:, e]
        return s
    g4 = dim // 4 * 4
    t = ((sq[:, 0:g4:4] + sq[:, 1:g4:4]) + sq[:, 2:g4:4]) + sq[:, 3:g4:4]
    for g in range(g4 // 4):
        s = s + t[:, g]
    for e in range(g4, dim):
        s = s + sq[:, e]
    return s


def range_query(cand, data, query, radius, metric=REF4, sqrt_out=True, max_candidates=0, max_results=0):
    """cand: candidate rows in candidate order (uncapped).  data: [n, dim] rows indexed by row id (or a callable
    row_ids -> rows).  Returns (rows u32, dist f32, n_within, n_candidates) ordered by (d2, position)."""
    cand = np.asarray(cand, dtype=np.uint32)
    n_candidates = len(cand)
    if max_candidates:
        cand = cand[:max_candidates]
    d2 = np.zeros(len(cand), np.float32)
    for c0 in range(0, len(cand), 1 << 16):          # (in slices: a C3 query has ~10^6 candidates of 3 KB)
        ids = cand[c0:c0 + (1 << 16)]
        x = data(ids) if callable(data) else np.asarray(data, dtype=np.float32)[ids]
        d2[c0:c0 + len(ids)] = l2_chain(x.reshape(len(ids), -1), query, metric)
    out = np.sqrt(d2) if sqrt_out else d2
    with np.errstate(invalid="ignore"):
        hit = out <= np.float32(radius)
    pos = np.nonzero(hit)[0]
    order = pos[np.lexsort((pos, d2[pos]))]
    n_within = len(order)
    if max_results:
        order = order[:max_results]
    return cand[order], out[order].astype(np.float32), n_within, n_candidates


def range_batch(oidx, data, queries, radius, nprobe, **kw):
    """-> (lims, rows, dist, n_within, n_candidates) in pqv_range_search's CSR form."""
    lims, rows, dist, nw, nc = [0], [], [], [], []
    for q in np.asarray(queries, dtype=np.float32):
        r, d, w, c = range_query(oidx.candidate_rows(q, nprobe), data, q, radius, **kw)
        rows.append(r); dist.append(d); nw.append(w); nc.append(c)
        lims.append(lims[-1] + len(r))
    cat = lambda xs, t: np.concatenate(xs).astype(t) if xs else np.zeros(0, t)   # noqa: E731
    return (np.array(lims, dtype=np.uint64), cat(rows, np.uint32), cat(dist, np.float32),
            np.array(nw, dtype=np.uint64), np.array(nc, dtype=np.uint64))
