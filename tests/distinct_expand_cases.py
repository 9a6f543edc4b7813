"""The fixtures of the expanding distinct / grouped top-k tests (no GPU): made once per process, shared by
tests/test_distinct_expand_host.py (which checks on the model that they are not dull) and tests/test_gpu_distinct_expand.py.

Base: 6 000 rows x dim 12, the oracle's index with 64 lists (seed 20261), a pool of 256 queries.  The group column ("doc") gives
1 - 8 rows per group; a group's rows lie near each other in list order (a jitter of +- 60 positions), so they are scattered over a
list and its neighbours and a probed prefix holds several chunks of one document.  A tenant ("org", 8 values) and the row masks are
attributes of the DOCUMENT (a mask then drops a quarter of the chosen documents' rows), as they are in a chunked corpus.

Each main case -- one per form -- takes 16 queries of the pool.  Two of them are built, on the model: query A's first P lists
hold exactly k groups of the case's row set and query B's exactly k - 1 (the row set -- validity, mask or a tenant value of its own
-- is rewritten inside those lists; for the shared row sets A's and B's lists are disjoint).  The others are picked from the pool
so that the batch has queries at p0 and queries whose distinct-count depth exceeds their row-count depth.  Everything is decided
by tests/distinct_expand_ref.py; nothing here looks at the code under test."""
import numpy as np

import distinct_expand_ref as dref
import distinct_filter_ref as fref
import expand_ref
from distinct_filter_ref import EQ, IN, RANGE

N, DIM, KC, NQ, POOL, SEED = 6000, 12, 64, 16, 256, 20261
TENANTS = 8

# form, k, nprobe, max_nprobe of the main cases
MAIN = {
    "none":  dict(form="none", k=20, nprobe=2, max_nprobe=8),      # no filter, no mask: a group column with NULLs
    "mask":  dict(form="mask", k=10, nprobe=2, max_nprobe=8),      # a shared row mask (1/8)
    "eq":    dict(form=EQ, k=6, nprobe=2, max_nprobe=16),
    "range": dict(form=RANGE, k=10, nprobe=1, max_nprobe=16),
    "in":    dict(form=IN, k=10, nprobe=2, max_nprobe=16),
}

_BASE = {}
_CASES = {}


def doc_mask(rng, group, sel):
    """a row mask of about `sel` of the rows: documents chosen with probability sel / 0.75, a quarter of their rows dropped"""
    vals = np.unique(group)
    chosen = vals[rng.random(len(vals)) < sel / 0.75]
    return np.isin(group, chosen) & (rng.random(len(group)) < 0.75)


def base(oracle):
    if "b" not in _BASE:
        rng = np.random.default_rng(SEED)
        data = rng.random((N, DIM), dtype=np.float32)
        pool = rng.random((POOL, DIM), dtype=np.float32)
        built = oracle.build_index(data, n_clusters=KC, max_iters=5, workers=1)
        lists = built.lists()
        order = np.concatenate(lists).astype(np.int64)
        near = np.argsort(np.arange(N) + rng.uniform(-60, 60, N), kind="stable")
        sizes = rng.integers(1, 9, N)
        ends = np.cumsum(sizes)
        ends = ends[: int(np.searchsorted(ends, N)) + 1]
        gid = np.searchsorted(ends, np.arange(N), side="right")          # run number of every slot of `near`
        vals = np.unique(rng.integers(-(2 ** 62), 2 ** 62, 4 * N))[: gid.max() + 1]
        rng.shuffle(vals)
        group = np.empty(N, np.int64)
        group[order[near]] = vals[gid]
        tenant_of = dict(zip(vals.tolist(), rng.integers(0, TENANTS, len(vals)).tolist()))
        tenant = np.array([tenant_of[g] for g in group.tolist()], np.int32)
        _BASE["b"] = dict(rng=rng, data=data, pool=pool, built=built, lists=lists, group=group, tenant=tenant,
                          valid4=doc_mask(rng, group, 1 / 4), mask8=doc_mask(rng, group, 1 / 8), mask64=doc_mask(rng, group, 1 / 64))
    return _BASE["b"]


def _region(b, q, P):
    return expand_ref.probe_order(b["built"], q, P).tolist()


def _pick_groups(b, rng, lists_of_region, count, free):
    """`count` groups with rows in the region, and all of their FREE rows there"""
    rows = np.concatenate([np.asarray(b["lists"][c]).astype(np.int64) for c in lists_of_region])
    rows = rows[free[rows]]
    gs = np.unique(b["group"][rows])
    assert len(gs) >= count, (len(gs), count)
    pick = rng.choice(gs, count, replace=False)
    return rows, rows[np.isin(b["group"][rows], pick)]


def case(oracle, name):
    """-> dict: queries [16, dim], k, nprobe, max_nprobe, group, gvalid, shared (bool rows or None), kind / spec / fvalues (filtered
    forms), M (None, 1-D or [16, n]: the row set besides the group validity), used (the model's nprobe_used), rows_used (the
    row-counting depth), total (gcnt(P) per query)"""
    if name in _CASES:
        return _CASES[name]
    b = base(oracle)
    c = dict(MAIN[name])
    k, p0, P, form = c["k"], c["nprobe"], c["max_nprobe"], c["form"]
    rng = np.random.default_rng(SEED + 1 + list(MAIN).index(name))
    pool, n = b["pool"], N
    regions = [_region(b, q, P) for q in pool]
    gvalid, shared, fvalues, spec_pool = None, None, None, None
    everything = np.ones(n, bool)
    A = 0
    if form in ("none", "mask"):
        # a shared row set: B's lists must not meet A's
        B = next(i for i in range(1, POOL) if not set(regions[i]) & set(regions[A]))
        allow = (b["valid4"] if form == "none" else b["mask8"]).copy()
        for i, cnt in ((A, k), (B, k - 1)):
            rows, keep = _pick_groups(b, rng, regions[i], cnt, everything)
            allow[rows] = False
            allow[keep] = True
        if form == "none":
            gvalid = allow
        else:
            shared = allow
        M_pool = [shared] * POOL
    else:
        B = 1
        fvalues = b["tenant"].copy()
        special = (100 + 10 * int(form), 101 + 10 * int(form))
        for i, cnt, t in ((A, k, special[0]), (B, k - 1, special[1])):
            _, keep = _pick_groups(b, rng, regions[i], cnt, fvalues < 100)
            fvalues[keep] = t
        t1 = rng.integers(0, TENANTS, POOL)
        t1[A], t1[B] = special
        if form == EQ:
            spec_pool = t1.tolist()
            spec_of = lambda idx: [spec_pool[i] for i in idx]
        elif form == RANGE:
            hi = np.where(t1 >= 100, t1, np.minimum(t1 + 1, TENANTS - 1))
            spec_pool = (t1.tolist(), hi.tolist())
            spec_of = lambda idx: ([spec_pool[0][i] for i in idx], [spec_pool[1][i] for i in idx])
        else:
            extra = rng.integers(0, TENANTS, (POOL, 2))
            spec_pool = [{int(t1[i])} if t1[i] >= 100 else {int(t1[i])} | set(extra[i, : i % 3].tolist()) for i in range(POOL)]
            spec_of = lambda idx: [spec_pool[i] for i in idx]
        all_idx = list(range(POOL))
        full = spec_of(all_idx)
        M_pool = [fref.allowed(fvalues, None, form, full, i, None) for i in range(POOL)]
    used = np.array([dref.nprobe_used(b["built"], b["lists"], b["group"], gvalid, M_pool[i], pool[i], k, p0, P) for i in range(POOL)])
    rows_used = np.array([dref.row_depth(b["built"], b["lists"], gvalid, M_pool[i], pool[i], k, p0, P) for i in range(POOL)])
    # the batch: A, B, up to three queries at p0, up to five whose distinct depth exceeds the row depth, then pool order
    p0_first = [i for i in np.flatnonzero(used == p0).tolist() if i not in (A, B)][:3]
    deeper = [i for i in np.flatnonzero(used > rows_used).tolist() if i not in (A, B) and i not in p0_first][:5]
    idx = [A, B] + p0_first + deeper
    idx += [i for i in range(POOL) if i not in idx][: NQ - len(idx)]
    c.update(name=name, idx=idx, queries=np.ascontiguousarray(pool[idx]), group=b["group"], gvalid=gvalid, shared=shared, fvalues=fvalues,
             kind=form if form not in ("none", "mask") else None, spec=spec_of(idx) if spec_pool is not None else None,
             M=None if form == "none" else shared if form == "mask" else np.stack([M_pool[i] for i in idx]),
             used=used[idx].astype(np.uint32), rows_used=rows_used[idx].astype(np.uint32),
             total=np.array([dref.gcnt(b["built"], b["lists"], b["group"], gvalid, M_pool[i], pool[i], P)[-1] for i in idx]))
    _CASES[name] = c
    return c


def dull(c):
    """the vacuity conditions of a main case -> the list of those that fail (empty: the fixture shows something)"""
    u, p0, P, k = c["used"], c["nprobe"], c["max_nprobe"], c["k"]
    out = []
    if len(set(u.tolist())) < 3:
        out.append("fewer than three values of nprobe_used")
    if not (u == p0).any() or not (u == P).any():
        out.append("p0 or P is not among the values")
    if not (c["total"] == k).any() or not (c["total"] == k - 1).any():
        out.append("no query with gcnt(P) == k or none with k - 1")
    if 4 * int((u > c["rows_used"]).sum()) < len(u):
        out.append("fewer than a quarter of the queries go deeper than the row count")
    return out
