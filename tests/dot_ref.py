"""numpy model of PQV_DOT (include/pqv.h): f32 arrays throughout, one numpy operation per rounded operation (numpy rounds every
f32 operation on its own: no fused multiply-add).

    s(q, x):   sum = 0; per full group of four dims t = ((q0 x0 + q1 x1) + q2 x2) + q3 x3, sum = sum + t; then the dim % 4 tail
               element by element, sum = sum + qe xe
    dist       0.0f - s          (never -0.0f: sum starts at +0.0f, and x + y is -0.0f only when both are)
    order      (dist, candidate position); on the device the key is (ord_bits(dist) << 32) | position

probe / candidates / topk_ref / range_ref restate a DOT call over (centroids, lists, rows): the centroids ranked ascending by
(dist, id), the probed lists' rows concatenated in probe order (a table: file after file, each file probed on its own), the cap
applied to candidate positions BEFORE an allow array, positions staying the unmasked ones."""
import numpy as np

EMPTY = 0xFFFFFFFF


def dot_chain(q, X):
    """s [m] f32 of rows X [m, dim] against q [dim] (or row by row against q [m, dim])."""
    x = np.ascontiguousarray(X, dtype=np.float32)
    qq = np.ascontiguousarray(q, dtype=np.float32)
    m, dim = x.shape
    p = (qq.reshape(1, -1) if qq.ndim < 2 else qq) * x
    s = np.zeros(m, dtype=np.float32)
    g4 = dim // 4 * 4
    t = ((p[:, 0:g4:4] + p[:, 1:g4:4]) + p[:, 2:g4:4]) + p[:, 3:g4:4]
    for g in range(g4 // 4):
        s = s + t[:, g]
    for e in range(g4, dim):
        s = s + p[:, e]
    return s


def dist(q, X):
    return np.float32(0.0) - dot_chain(q, X)


def ord_bits(d):
    """the order-preserving map of f32 bits to u32: ascending ord_bits == ascending values (-0.0 below +0.0)"""
    b = np.ascontiguousarray(d, dtype=np.float32).view(np.uint32)
    return b ^ np.where(b >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000)).astype(np.uint32)


def probe(q, centroids, nprobe):
    """centroid ids ranked ascending by (dist(q, centroid), id), the first min(nprobe, n_clusters)"""
    c = np.ascontiguousarray(centroids, dtype=np.float32)
    if len(c) == 0:
        return np.zeros(0, np.int64)
    o = ord_bits(dist(q, c))
    return np.lexsort((np.arange(len(c)), o))[:min(nprobe, len(c))]


def candidates(q, centroids, lists, nprobe, files=None):
    """candidate rows in candidate order (uncapped).  files: [(centroids_f, lists_f, row_base_f)] -- the table's file-major form,
    every file probed on its own with `nprobe`; centroids / lists are ignored then."""
    if files is None:
        files = [(centroids, lists, 0)]
    out = []
    for cf, lf, base in files:
        for c in probe(q, cf, nprobe):
            out.append(np.asarray(lf[c], dtype=np.int64) + base)
    return np.concatenate(out).astype(np.uint32) if out else np.zeros(0, np.uint32)


def _considered(q, centroids, lists, rows, nprobe, max_candidates, allow, files):
    cand = candidates(q, centroids, lists, nprobe, files)
    n_candidates = len(cand)
    pos = np.arange(len(cand))
    if max_candidates:
        cand, pos = cand[:max_candidates], pos[:max_candidates]
    if allow is not None:
        keep = np.asarray(allow, dtype=bool)[cand.astype(np.int64)]
        cand, pos = cand[keep], pos[keep]
    d = dist(q, np.asarray(rows, dtype=np.float32)[cand.astype(np.int64)].reshape(len(cand), -1)) if len(cand) else np.zeros(0, np.float32)
    return cand, pos, d, n_candidates


def topk_ref(q, centroids, lists, rows, k, nprobe, max_candidates=0, allow=None, files=None):
    """-> (rows u32 [k], dist f32 [k], n_found, n_candidates); entries past n_found are 0xFFFFFFFF / +inf"""
    cand, pos, d, nc = _considered(q, centroids, lists, rows, nprobe, max_candidates, allow, files)
    order = np.lexsort((pos, ord_bits(d)))[:k]
    orow = np.full(k, EMPTY, dtype=np.uint32)
    od = np.full(k, np.inf, dtype=np.float32)
    orow[:len(order)] = cand[order]
    od[:len(order)] = d[order]
    return orow, od, len(order), nc


def range_ref(q, centroids, lists, rows, radius, nprobe, max_candidates=0, max_results=0, allow=None, files=None):
    """-> (rows u32, dist f32, n_within, n_candidates): the candidates with dist <= radius, ascending by (dist, position)"""
    cand, pos, d, nc = _considered(q, centroids, lists, rows, nprobe, max_candidates, allow, files)
    with np.errstate(invalid="ignore"):
        hit = np.nonzero(d <= np.float32(radius))[0]
    order = hit[np.lexsort((pos[hit], ord_bits(d[hit])))]
    n_within = len(order)
    if max_results:
        order = order[:max_results]
    return cand[order], d[order].astype(np.float32), n_within, nc


def topk_batch(queries, centroids, lists, rows, k, nprobe, **kw):
    res = [topk_ref(q, centroids, lists, rows, k, nprobe, **kw) for q in np.asarray(queries, dtype=np.float32)]
    return (np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.array([r[2] for r in res], np.uint32),
            np.array([r[3] for r in res], np.uint64))


def range_batch(queries, centroids, lists, rows, radius, nprobe, **kw):
    """-> (lims, rows, dist, n_within, n_candidates) in pqv_range_search's CSR form"""
    lims, orow, od, nw, nc = [0], [], [], [], []
    for q in np.asarray(queries, dtype=np.float32):
        r, d, w, c = range_ref(q, centroids, lists, rows, radius, nprobe, **kw)
        orow.append(r); od.append(d); nw.append(w); nc.append(c)
        lims.append(lims[-1] + len(r))
    cat = lambda xs, t: np.concatenate(xs).astype(t) if xs else np.zeros(0, t)   # noqa: E731
    return (np.array(lims, dtype=np.uint64), cat(orow, np.uint32), cat(od, np.float32), np.array(nw, dtype=np.uint64),
            np.array(nc, dtype=np.uint64))
