"""The shapes, inputs and CPU references of the multi-chunk row tests (tests/test_gpu_long_rows.py on the GPU,
tests/test_long_rows_host.py without one).

A shape is a dimension, a metric and a searcher layout chosen so that the exact-distance tile of the masked kernel family runs
its chunk loop `for (c0 = 0; c0 < G; c0 += CG)` more than once: chunk_plan() restates the storage padding rule of
pqv_searcher_create and the CG rule of launch_masked_s (the same in launch_distinct_s, launch_grouped_s and, without SEQ, in
launch_dot_s) and SHAPES["sees"] states what the kernel must see -- a change of either rule makes both test modules fail.

Case holds one shape's inputs -- the rows and queries test_gpu_mask.Setup draws from its seed, an oracle-built index whose lists
reshape_lists() re-cuts (one list of 40 rows, one of more than 512), two row masks and the key columns -- and the references
of every call, each a restatement already under tests/ (mask_ref, key_filter_ref, distinct_ref, grouped_ref, dot_ref,
cosine_ref over range_oracle.l2_chain) run over the C oracle's candidate_rows.  Nothing here needs a GPU.

Ties: a seed is chosen (by search, on the CPU) so that for every query the distances of ALL rows are pairwise distinct
(Case.assert_distinct) -- every call's considered rows are a subset -- so the order (distance, position) never consults the
position and the reference's heap history plays no part.  That is a condition on the inputs; no comparison has a tolerance."""
import numpy as np

import cosine_ref
import distinct_ref
import dot_ref
import grouped_ref
import key_filter_ref
import mask_ref
from range_oracle import REF4, SEQ, l2_chain

EMPTY = 0xFFFFFFFF
N, KC, NQ = 1500, 5, 5
NPROBES = (2, KC)

# name -> dim, metric of the chain (REF4 / SEQ), kind ("l2": the metric itself, "cos": PQV_COSINE, "dot": PQV_DOT), layout, seed,
# and what the kernel sees: (G, CG, chunk sizes, tail)
SHAPES = {
    "192":        dict(dim=192, metric=REF4, kind="l2", row_order=False, seed=1003, sees=(48, 32, [32, 16], 0)),
    "132":        dict(dim=132, metric=REF4, kind="l2", row_order=False, seed=1013, sees=(33, 32, [32, 1], 0)),
    "260-row":    dict(dim=260, metric=REF4, kind="l2", row_order=True, seed=1003, sees=(65, 32, [32, 32, 1], 0)),
    "260":        dict(dim=260, metric=REF4, kind="l2", row_order=False, seed=1003, sees=(80, 32, [32, 32, 16], 0)),
    "768":        dict(dim=768, metric=REF4, kind="l2", row_order=False, seed=1062, sees=(192, 64, [64, 64, 64], 0)),
    "134":        dict(dim=134, metric=REF4, kind="l2", row_order=False, seed=1011, sees=(33, 32, [32, 1], 2)),
    "3":          dict(dim=3, metric=REF4, kind="l2", row_order=False, seed=1000, sees=(0, 32, [], 3)),
    "96-seq-row": dict(dim=96, metric=SEQ, kind="l2", row_order=True, seed=1011, sees=(24, 16, [16, 8], 0)),
    "96-seq":     dict(dim=96, metric=SEQ, kind="l2", row_order=False, seed=1011, sees=(32, 16, [16, 16], 0)),
    "70-seq":     dict(dim=70, metric=SEQ, kind="l2", row_order=False, seed=1000, sees=(17, 16, [16, 1], 2)),
    "132-cos":    dict(dim=132, metric=REF4, kind="cos", row_order=False, seed=1004, sees=(33, 32, [32, 1], 0)),
    "768-cos":    dict(dim=768, metric=REF4, kind="cos", row_order=False, seed=1042, sees=(192, 64, [64, 64, 64], 0)),
    "132-dot":    dict(dim=132, metric=REF4, kind="dot", row_order=False, seed=1005, sees=(33, 32, [32, 1], 0)),
    "134-dot":    dict(dim=134, metric=REF4, kind="dot", row_order=False, seed=1023, sees=(33, 32, [32, 1], 2)),
    "768-dot":    dict(dim=768, metric=REF4, kind="dot", row_order=False, seed=3087, sees=(192, 64, [64, 64, 64], 0)),
}
L2_SHAPES = [n for n, c in SHAPES.items() if c["kind"] == "l2"]
COS_SHAPES = [n for n, c in SHAPES.items() if c["kind"] == "cos"]
DOT_SHAPES = [n for n, c in SHAPES.items() if c["kind"] == "dot"]


def stored_dim(dim, row_order):
    """The storage dimension of a searcher's rows (pqv_searcher_create): in the default layout a dim that is a multiple of 4 but
    not of 64 is zero-padded to the cheapest of a multiple of 256 (dim >= 192 only), 128 or 64 that stays within 4/3 of dim."""
    if row_order or dim % 4 or dim % 64 == 0:
        return dim
    up = lambda m: (dim + m - 1) // m * m       # noqa: E731
    lim = dim * 4 // 3
    if dim >= 192 and up(256) <= lim:
        return up(256)
    if up(128) <= lim:
        return up(128)
    if up(64) <= lim:
        return up(64)
    return dim


def chunk_plan(dim, metric, row_order):
    """-> (stored dim, G, CG, [float4 groups of every turn of the chunk loop], tail, aligned): launch_masked_s on the stored dim."""
    sdim = stored_dim(dim, row_order)
    aligned = sdim % 4 == 0
    g = sdim // 4
    if metric == SEQ:
        cg = 16
    elif aligned and g >= 64 and g % 64 == 0:
        cg = 64
    else:
        cg = 32
    return sdim, g, cg, [min(cg, g - c0) for c0 in range(0, g, cg)], sdim % 4, aligned


def plan_of(name):
    c = SHAPES[name]
    return chunk_plan(c["dim"], c["metric"], c["row_order"])


def reshape_lists(lists):
    """The lists= hook of test_gpu_mask.Setup: list 0 keeps 40 rows (a flush tile with nvalid < 64 in every probe of it), list 2
    keeps 100, list 1 takes the rest of both (more than 512 rows: several blocks, four waves)."""
    l = [np.asarray(x, np.uint32) for x in lists]
    assert len(l) == KC and len(l[0]) > 40 and len(l[2]) > 100
    return [l[0][:40], np.concatenate([l[1], l[0][40:], l[2][100:]]), l[2][:100], l[3], l[4]]


def wide(v):
    """an int64 image of small key values whose high and low words both matter (and negative for small v)"""
    return np.asarray(v, dtype=np.int64) * np.int64(2 ** 33 + 1) - np.int64(2 ** 40)


def draw(seed, dim):
    """(rows, queries) as test_gpu_mask.Setup draws them from `seed`"""
    rng = np.random.default_rng(seed)
    return rng.random((N, dim), dtype=np.float32), rng.random((NQ, dim), dtype=np.float32)


def all_distances(kind, metric, data, queries):
    """[NQ, n] f32: every row's distance to every query before the output transform (d2; PQV_COSINE: d2 of the normalised
    vectors; PQV_DOT: 0 - s)"""
    if kind == "dot":
        return np.stack([dot_ref.dist(q, data) for q in queries])
    if kind == "cos":
        data, queries = cosine_ref.normalise(data), cosine_ref.normalise(queries)
    return np.stack([l2_chain(data, q, metric) for q in queries])


def distinct_per_query(d):
    return all(len(np.unique(np.ascontiguousarray(row).view(np.uint32))) == len(row) for row in d)


def _pad(rows, dist, k):
    r = np.full(k, EMPTY, np.uint32)
    d = np.full(k, np.inf, np.float32)
    r[:len(rows)], d[:len(rows)] = rows, dist
    return r, d


class Case:
    """One shape's inputs and references.  parts: (rows, queries, centroids, lists) of a live Setup -- checked against draw() --
    or None: the index is built here with the oracle, as Setup builds it."""

    def __init__(self, name, oracle, parts=None):
        c = SHAPES[name]
        self.name, self.dim, self.metric, self.kind, self.seed = name, c["dim"], c["metric"], c["kind"], c["seed"]
        data, queries = draw(self.seed, self.dim)
        if parts is None:
            built = oracle.build_index(data, n_clusters=KC, max_iters=5, workers=1)
            centroids, lists = built.centroids, reshape_lists(built.lists())
        else:
            assert (parts[0] == data).all() and (parts[1] == queries).all(), "the Setup drew other inputs than draw()"
            centroids, lists = parts[2], [np.asarray(l, np.uint32) for l in parts[3]]
        self.data, self.queries, self.centroids, self.lists = data, queries, np.asarray(centroids, np.float32), lists
        self.n = N
        # what the chains run on: the vectors themselves, or (PQV_COSINE) their float32 normalisation
        norm = cosine_ref.normalise if self.kind == "cos" else (lambda x: x)
        self.rdata, self.rq = norm(data), norm(queries)
        self.oidx = oracle.index_from_parts(self.dim, norm(self.centroids.reshape(-1, self.dim)), lists)
        aux = np.random.default_rng(self.seed + 7919)
        self.masks = {"1/64": aux.random(N) < 1 / 64, "1/2": aux.random(N) < 1 / 2}
        self.tenant = aux.integers(0, 4, N).astype(np.int32)                 # keyed calls: a quarter of the rows per key
        self.tenant_valid = (aux.random(N) >= 0.2).astype(np.uint8)          # ... on a null-carrying column
        self.group = aux.integers(0, N // 16, N).astype(np.int32)            # grouped calls: about 16 rows per key
        self.group_valid = (aux.random(N) >= 0.1).astype(np.uint8)
        self._cand = {}

    # ---- conditions on the inputs ------------------------------------------------------------------------------------
    def assert_lists(self):
        lens = [len(l) for l in self.lists]
        assert len(lens) == KC and sum(lens) == N and min(lens) < 64 and max(lens) > 512, lens
        assert len(np.unique(np.concatenate(self.lists))) == N

    def assert_distinct(self):
        assert distinct_per_query(all_distances(self.kind, self.metric, self.data, self.queries)), \
            f"shape {self.name}, seed {self.seed}: two rows are equally far from one query"

    # ---- candidates --------------------------------------------------------------------------------------------------
    def cand(self, qi, nprobe):
        if (qi, nprobe) not in self._cand:
            if self.kind == "dot":
                self._cand[qi, nprobe] = dot_ref.candidates(self.queries[qi], self.centroids.reshape(-1, self.dim), self.lists, nprobe)
            else:
                self._cand[qi, nprobe] = self.oidx.candidate_rows(self.rq[qi], nprobe)
        return self._cand[qi, nprobe]

    def _allow(self, allowed, qi):
        """allowed: one array for the call, a list of NQ arrays (per-query filters), or None (an unmasked call)"""
        if allowed is None:
            return np.ones(N, bool)
        return np.asarray(allowed[qi] if isinstance(allowed, (list, tuple)) else allowed, bool)

    def _out(self, d, sqrt_out):
        if self.kind == "cos":
            return cosine_ref.half(d)
        return np.sqrt(d) if sqrt_out and self.kind == "l2" else d

    # ---- references --------------------------------------------------------------------------------------------------
    def topk(self, allowed, k, nprobe, sqrt_out=False):
        """-> (rows [NQ, k] u32, dist [NQ, k] f32, n_found u32, n_candidates u64, tie flags u32): the masked / keyed / unmasked
        top-k.  dist is d2, sqrt(d2) (sqrt_out), 0.5 d2 (PQV_COSINE) or 0 - s (PQV_DOT).  The tie flag is pqv.h's: two of the k
        results, or the k-th and the runner-up, have equal output distance; with sqrt_out that must not happen (the reference
        then orders by heap history, which (d2, position) does not restate) and is asserted here."""
        rows, dist = np.empty((NQ, k), np.uint32), np.empty((NQ, k), np.float32)
        nf, nc, tf = np.zeros(NQ, np.uint32), np.zeros(NQ, np.uint64), np.zeros(NQ, np.uint32)
        for qi in range(NQ):
            allow = self._allow(allowed, qi)
            if self.kind == "dot":
                r, d, n, c = dot_ref.topk_ref(self.queries[qi], self.centroids.reshape(-1, self.dim), self.lists, self.data, k + 1, nprobe,
                                              allow=allow)
                r, d = r[:n], d[:n]
            else:
                r, d, c, _ = mask_ref.masked_topk(self.cand(qi, nprobe), allow, self.rdata, self.rq[qi], k + 1, metric=self.metric)
            d = self._out(d, sqrt_out)
            tf[qi] = len(np.unique(d)) < len(d)
            assert not (sqrt_out and tf[qi]), f"shape {self.name}: equal sqrt distances among the first {k + 1} of query {qi}"
            rows[qi], dist[qi] = _pad(r[:k], d[:k], k)
            nf[qi], nc[qi] = min(len(r), k), c
        if self.kind == "dot":
            tf[:] = 0           # (PQV_DOT has no heap to replay: the flags are written with zeros)
        return rows, dist, nf, nc, tf

    def range(self, allowed, radius, nprobe, sqrt_out=True, max_results=0):
        """-> (lims, rows, dist, n_within, n_candidates) in pqv_range_search's CSR form"""
        lims, rows, dist, nw, nc = [0], [], [], [], []
        for qi in range(NQ):
            allow = self._allow(allowed, qi)
            if self.kind == "dot":
                r, d, w, c = dot_ref.range_ref(self.queries[qi], self.centroids.reshape(-1, self.dim), self.lists, self.data, radius, nprobe,
                                               max_results=max_results, allow=allow)
            else:
                r, d, w, c = mask_ref.masked_range(self.cand(qi, nprobe), allow, self.rdata, self.rq[qi], radius, metric=self.metric,
                                                   sqrt_out=sqrt_out, max_results=max_results, halve=self.kind == "cos")
            rows.append(r); dist.append(d); nw.append(w); nc.append(c)
            lims.append(lims[-1] + len(r))
        return (np.array(lims, np.uint64), np.concatenate(rows).astype(np.uint32), np.concatenate(dist).astype(np.float32),
                np.array(nw, np.uint64), np.array(nc, np.uint64))

    def radius(self, allowed, nprobe, sqrt_out=True, rank=40):
        """the output distance of about the rank-th nearest considered row of query 0 (fewer considered rows: the middle one)"""
        _, d, nf, _, _ = self.topk(allowed, rank, nprobe)
        assert nf[0] > 0
        d = d[0, min(rank - 1, int(nf[0]) // 2)]
        return float(np.sqrt(d) if sqrt_out and self.kind == "l2" else d)

    def key_allowed(self, values, valid, kind, a, b, shared=None):
        """[NQ allow arrays] of a per-query key filter (key_filter_ref)"""
        return [key_filter_ref.allowed_for(values, valid, kind, a, b, qi, shared) for qi in range(NQ)]

    def distinct(self, column, valid, mask, k, nprobe):
        """-> (rows [NQ, k], d2 [NQ, k], keys [NQ, k] i64, n_found, n_candidates): distinct_ref over the oracle's candidates"""
        rows, dist, keys = np.full((NQ, k), EMPTY, np.uint32), np.full((NQ, k), np.inf, np.float32), np.zeros((NQ, k), np.int64)
        nf, nc = np.zeros(NQ, np.uint32), np.zeros(NQ, np.uint64)
        for qi in range(NQ):
            r, d, g, c, _ = distinct_ref.distinct_topk(self.cand(qi, nprobe), column, valid, mask, self.rdata, self.rq[qi], k,
                                                       metric=self.metric)
            rows[qi, :len(r)], dist[qi, :len(r)], keys[qi, :len(r)], nf[qi], nc[qi] = r, d, g, len(r), c
        return rows, dist, keys, nf, nc

    def grouped(self, column, valid, mask, k, m, nprobe):
        """-> (rows [NQ, k, m], d2 [NQ, k, m], keys [NQ, k] i64, group_rows [NQ, k], n_found, n_candidates): grouped_ref"""
        res = [grouped_ref.grouped_topk(self.cand(qi, nprobe), column, valid, mask, self.rdata, self.rq[qi], k, m, metric=self.metric)
               for qi in range(NQ)]
        return (np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.stack([r[2] for r in res]),
                np.stack([r[3] for r in res]), np.array([r[4] for r in res], np.uint32), np.array([r[5] for r in res], np.uint64))


# the per-query filters of the keyed cases, on the tenant column's small values (v -> wide(v) on the int64 column)
QUERY_KEYS = [0, 1, 2, 3, 2]
QUERY_RANGES = ([0, 1, 2, 0, 3], [1, 3, 2, 3, 0])            # (lo, hi) inclusive; the last query's is empty (lo > hi)
QUERY_SETS = [[0, 2], [1], [0, 1, 2, 3], [3, 7], []]          # 7 is no key of the column; the last query's set is empty
