"""A zoo of MUTATED indexes and the numpy expectation of every search mode on them (test infrastructure: nothing here calls the
library under test).

A case is a corpus X that grows twice (n0 -> n1 -> n2 rows) and five index states over it, each derived from the one before by the
numpy models of tests/append_ref.py and tests/remove_ref.py:

    built      oracle.build_index(X[:n0])                                   the baseline
    appended   + rows [n0, n1)                                              device lists, permutation_of carried over
    removed    flags remove ~35 % at random, EVERY row of list `emptied`    fewer list rows than corpus rows, an empty list, the
               and the newest 30 rows                                       bound above the largest id
    chained    + rows [n1, n2), then remove(rows=) of 500 ids in messy      several generations of device lists (the emptied list
               order -- the new rows of list `emptied` among them           stays empty)
    compacted  compact of chained                                           renumbered ids, columns re-made as column[old_row]

Per-row columns (one value per corpus row, n2 of them): tenant int32 -- two common values, eight "mid" ones and four "tiny" ones of six
rows each, so that a per-query tenant filter leaves some queries k rows inside nprobe lists, some only after more lists and some
never --, ts int64 = TS0 + 1000 * tenant + noise with a validity array (10 % NULL), doc int32 (about five rows per document: the
group column).  Masks over corpus rows: `dense` (every other row at random; it allows removed rows and rows past every bound) and
`sparse` (0.1 % of the rows nearest to most of the centroids, 30 % of the others: the number of lists a query needs for k
allowed rows depends on where it lies).  32 queries, most of them beside a corpus row of one list after the other: query 0 is the
centroid of the emptied list, query 1 a copy of a removed row.

expect(model, spec) is the numpy answer of one call, put together from the references the project has: the oracle's top-k and
candidate order, range_oracle, cosine_ref, dot_ref, mask_ref, key_filter_ref, expand_ref, depth_ref, distinct_ref, grouped_ref,
distinct_filter_ref and distinct_expand_ref."""
import numpy as np

import append_ref
import assign_exact  # noqa: F401  (append_ref's assignment: the exact nearest centroid)
import cosine_ref
import depth_ref
import distinct_expand_ref
import distinct_filter_ref
import distinct_ref
import dot_ref
import expand_ref
import grouped_ref
import mask_ref
import range_oracle
import remove_ref
from key_filter_ref import EQ, IN, RANGE
from range_oracle import REF4, SEQ, l2_chain

EMPTY = 0xFFFFFFFF
K, NPROBE, M = 10, 4, 3
CAP = 150                         # a max_candidates below every query's candidate count
TS0 = 1 << 40
STATES = ["built", "appended", "removed", "chained", "compacted"]
MUTATED = ["appended", "removed", "chained", "compacted"]

# nprobe_f / max_nprobe: the depths of the filtered and expanding calls; mid_f: the share of rows of one "mid" tenant, between
# K / (rows of max_nprobe - 1 lists) and K / (rows of nprobe_f lists) of every state
SHAPES = {
    "screened": dict(dim=64, kc=16, n0=6144, n1=8192, n2=9216, integer=False, nprobe_f=2, max_nprobe=6, mid_f=0.008, seed=64),
    "exact30": dict(dim=30, kc=7, n0=2000, n1=2600, n2=2900, integer=False, nprobe_f=1, max_nprobe=4, mid_f=0.025, seed=30),
    "padded72": dict(dim=72, kc=24, n0=3000, n1=3800, n2=4200, integer=False, nprobe_f=2, max_nprobe=8, mid_f=0.025, seed=72),
    "int8_256": dict(dim=256, kc=8, n0=3072, n1=4096, n2=4608, integer=False, nprobe_f=1, max_nprobe=4, mid_f=0.012, seed=256),
    "ties": dict(dim=64, kc=16, n0=6144, n1=8192, n2=9216, integer=True, nprobe_f=2, max_nprobe=6, mid_f=0.008, seed=65),
    # every depth the modes use (1, 2, 4 and max_nprobe) is <= kc / 4: the screened centroid probe is eligible in every call, the
    # expanding ones included (tests/test_gpu_probe_screen_modes.py; not one of CASES)
    "probe32": dict(dim=64, kc=32, n0=12288, n1=16384, n2=18432, integer=False, nprobe_f=2, max_nprobe=8, mid_f=0.004, seed=66),
    # the workload's row length, and the cases tests/far_rows_cases.py relocates onto rows beyond 2^31 / 2^32 bytes and elements of a
    # 16 GiB corpus (tests/test_gpu_far_rows.py; not among CASES): a multiple of 64 dims and a mean list of >= 192 rows in every
    # state -- the images-only layout --, the full mode set; far768i: the same sizes with distances that tie.  (radius_cuts_all:
    # pick_radius)
    "far768": dict(dim=768, kc=8, n0=3072, n1=4096, n2=4608, integer=False, nprobe_f=1, max_nprobe=4, mid_f=0.012, seed=768,
                   radius_cuts_all=False),
    "far768i": dict(dim=768, kc=8, n0=3072, n1=4096, n2=4608, integer=True, nprobe_f=1, max_nprobe=4, mid_f=0.012, seed=769,
                    radius_cuts_all=False),
}
CASES = ["screened", "exact30", "padded72", "int8_256", "ties"]          # what test_gpu_mutated_search.py / _table.py run
N_MID, N_TINY, TINY_ROWS = 8, 4, 6
MID0, TINY0 = 2, 2 + N_MID           # tenants 0, 1: common; 2 .. 9: mid; 10 .. 13: tiny


class Model:
    """One state: the lists, the rows they index (X: by row id), the columns and masks over those rows."""

    def __init__(self, case, name, lists, X, cols, masks, old_row=None):
        self.case, self.name, self.lists, self.X, self.cols, self.masks, self.old_row = case, name, lists, X, cols, masks, old_row
        self.dim, self.C = case.dim, case.C
        self.n = len(X)
        self.bound = None                # the carried row bound, set by the case
        self._memo = {}

    def oidx(self, oracle, metric="l2"):
        """the oracle index a metric probes: the centroids (cosine: normalised) and this state's lists"""
        key = ("oidx", metric)
        if key not in self._memo:
            C = cosine_ref.normalise(self.C) if metric == "cos" else self.C
            self._memo[key] = oracle.index_from_parts(self.dim, C, self.lists)
        return self._memo[key]

    def rows_for(self, metric):
        if metric != "cos":
            return self.X
        if "Xn" not in self._memo:
            self._memo["Xn"] = cosine_ref.normalise(self.X)
        return self._memo["Xn"]

    def in_lists(self):
        a = np.zeros(self.n, bool)
        for l in self.lists:
            a[np.asarray(l, np.int64)] = True
        return a


class Case:
    def __init__(self, oracle, name):
        sh = SHAPES[name]
        self.name = name
        self.dim, self.kc, self.n0, self.n1, self.n2 = sh["dim"], sh["kc"], sh["n0"], sh["n1"], sh["n2"]
        self.nprobe_f, self.max_nprobe = sh["nprobe_f"], sh["max_nprobe"]
        self.integer = sh["integer"]         # small integers: distances tie, and every chain of partial sums is exact
        rng = np.random.default_rng(sh["seed"])
        draw = (lambda n: rng.integers(0, 3, (n, self.dim)).astype(np.float32)) if sh["integer"] else \
               (lambda n: rng.random((n, self.dim), dtype=np.float32))
        self.X = X = draw(self.n2)
        n0, n1, n2 = self.n0, self.n1, self.n2

        # the states --------------------------------------------------------------------------------------------------------
        base = oracle.build_index(X[:n0], n_clusters=self.kc, max_iters=5, workers=1)
        self.C = base.centroids
        built = base.lists()
        appended, assign1 = append_ref.append_lists(built, X, self.C, n0, n1 - n0)
        self.emptied = e = int(np.argmin([len(l) for l in appended]))
        flags = rng.random(n1) < 0.35
        flags[np.asarray(appended[e], np.int64)] = True
        flags[n1 - 30:] = True
        self.flags = flags
        removed = remove_ref.remove(appended, flags)
        self.grown, assign2 = append_ref.append_lists(removed, X, self.C, n1, n2 - n1)        # (an intermediate index, not searched)
        mine = np.asarray(self.grown[e], np.int64)                                            # the emptied list's new rows
        others = rng.choice(np.setdiff1d(np.arange(n2), mine), 500 - len(mine), replace=False)
        gone = rng.permutation(np.concatenate([mine, others])).astype(np.uint32)
        self.gone = np.concatenate([gone, gone[:7], np.array([n2 + 5, EMPTY], np.uint32)])    # any order, duplicates, unindexed ids
        chained = remove_ref.remove_rows(self.grown, self.gone)
        X_new, compacted, old_row = remove_ref.compact(chained, X)
        self.old_row = old_row
        assert len(removed[e]) == 0 and len(chained[e]) == 0 and append_ref.row_bound(removed) < n1

        # columns and masks over the n2 corpus rows -------------------------------------------------------------------------
        p = np.zeros(TINY0)
        p[MID0:] = sh["mid_f"]
        p[0], p[1] = 0.6 * (1 - p.sum()), 0.4 * (1 - p.sum())
        tenant = rng.choice(TINY0, n2, p=p).astype(np.int32)
        tiny_rows = rng.choice(n1, N_TINY * TINY_ROWS, replace=False)
        tenant[tiny_rows] = np.repeat(np.arange(TINY0, TINY0 + N_TINY), TINY_ROWS).astype(np.int32)
        ts = (TS0 + 1000 * tenant.astype(np.int64) + rng.integers(0, 1000, n2)).astype(np.int64)
        ts_valid = rng.random(n2) >= 0.1
        doc = rng.integers(0, n2 // 5, n2).astype(np.int32)
        cols = {"tenant": (tenant, None), "ts": (ts, ts_valid), "doc": (doc, None)}
        assign = np.zeros(n2, np.int64)
        for c, l in enumerate(built):
            assign[np.asarray(l, np.int64)] = c
        assign[n0:n1], assign[n1:] = assign1, assign2
        thin = np.zeros(self.kc, bool)
        thin[rng.permutation(self.kc)[:self.kc - max(2, self.kc // 5)]] = True
        thin[e] = True
        self.thin_lists = thin
        masks = {"dense": rng.random(n2) < 0.5, "sparse": rng.random(n2) < np.where(thin[assign], 0.001, 0.3)}

        def model(name, lists, bound):
            m = Model(self, name, lists, X, cols, masks)
            m.bound = bound
            return m
        self.models = {"built": model("built", built, n0), "appended": model("appended", appended, n1),
                       "removed": model("removed", removed, n1), "chained": model("chained", chained, n2)}
        at = old_row.astype(np.int64)
        self.models["compacted"] = Model(self, "compacted", compacted, X_new, {n: (v[at], None if ok is None else ok[at]) for n, (v, ok) in cols.items()},
                                         {n: a[at] for n, a in masks.items()}, old_row)
        self.models["compacted"].bound = len(old_row)

        # queries and their filters ---------------------------------------------------------------------------------------------
        def queries(nq):
            # three of four queries lie beside a corpus row, one row of every list in turn -- uniform queries all sit near the
            # middle of the cube and probe the same few central lists --, the fourth is uniform
            Q = draw(nq)
            for i in range(nq):
                if i % 4 != 3:
                    l = appended[i % self.kc]
                    Q[i] = X[int(l[(7 * i) % len(l)])]
                    if sh["integer"]:
                        Q[i, rng.choice(self.dim, 8, replace=False)] = rng.integers(0, 3, 8).astype(np.float32)
                    else:
                        Q[i] += np.float32(0.05) * (rng.random(self.dim, dtype=np.float32) - np.float32(0.5))
            Q[0] = self.C[e]
            Q[1] = X[int(np.nonzero(flags[:n0] & (assign[:n0] != e))[0][5])]
            return np.ascontiguousarray(Q, np.float32)
        self.Q = queries(32)
        self.Q160 = queries(160) if name == "screened" else None
        classes = [0, MID0, TINY0, MID0 + 1, 1, MID0 + 2, TINY0 + 1, MID0 + 3, MID0 + 4, MID0 + 5, TINY0 + 2, MID0 + 6, MID0 + 7, TINY0 + 3]
        self.qkeys = np.array([classes[i % len(classes)] for i in range(160)], np.int64)
        self.qkeys[1] = int(tenant[int(np.nonzero(flags[:n0] & (assign[:n0] != e))[0][5])])   # query 1: the key of the removed row it copies
        self.filters = {
            "eq": ("tenant", EQ, self.qkeys),
            "in": ("tenant", IN, [{int(t), TINY0 + (i % N_TINY), 999999} for i, t in enumerate(self.qkeys)]),
            "range": ("ts", RANGE, (TS0 + 1000 * self.qkeys, TS0 + 1000 * self.qkeys + 999)),
            "eq64": ("ts", EQ, np.array([int(ts[(17 * i) % n0]) for i in range(160)], np.int64)),
        }

    def queries(self, spec):
        Q = self.Q160 if spec.get("q160") else self.Q
        return Q[:spec.get("nq", len(Q))]

    def filter_of(self, name, nq):
        """-> (column name, kind, the spec cut to nq queries)"""
        col, kind, spec = self.filters[name]
        if kind == RANGE:
            return col, kind, (spec[0][:nq], spec[1][:nq])
        return col, kind, spec[:nq]


_MADE = {}


def case(oracle, name):
    if name not in _MADE:
        _MADE[name] = Case(oracle, name)
    return _MADE[name]


# ---- call specs --------------------------------------------------------------------------------------------------------------------
# A spec names one call: call (topk | topk_device | range | distinct | grouped | distinct_device | grouped_device), k, nprobe,
# metric (l2 | cos | dot), mask (a mask's name, or a bool array over the rows), filt (a filter's name), maxc (max_candidates), maxr (max_results), maxp (max_nprobe),
# nq (the first nq queries), q160 (the 160-query batch), radius (filled in by expect()).
# A DEPTH spec (pqv_topk_depth: the plain call under per-query probe depths) carries maxp and one of depths (uint32 [nq], the given
# depths) and ratio (a float, or RESOLVE until resolve() fills it in per state: ratio_for).
RESOLVE = "to be resolved"


def is_depth(sp):
    return sp.get("depths") is not None or sp.get("ratio") is not None


def spec(call, **kw):
    s = dict(call=call, k=K, nprobe=NPROBE, metric="l2", mask=None, filt=None, maxc=0, maxr=0, maxp=None, nq=None, q160=False, m=M,
             depths=None, ratio=None)
    s.update(kw)
    if is_depth(s):
        assert s["maxp"] and (s["depths"] is None or s["ratio"] is None) and s["mask"] is None and not s["filt"] and not s["maxc"]
        assert call in ("topk", "topk_device")
    # pqv_topk as the reference runs it: sqrt_out, whose final stable sort is by sqrt(d2) -- two d2 that round to one sqrt keep
    # the heap's order (the oracle's topk_batch); every other call returns d2 (cosine / dot: the output distance).  A depth call
    # follows the plain call: query q's answer is the uniform call's at nprobe_used[q] (pqv.h)
    s["sqrt"] = call == "topk" and s["metric"] == "l2" and not (s["mask"] is not None or s["filt"] or s["maxc"] is None or s["maxc"]
                                                                 or (s["maxp"] and not is_depth(s)))
    return s


def allowed_rows(model, sp, nq):
    """None (every row), or bool [n] / [nq, n]: the rows query q may consider -- the call's mask AND its per-query filter"""
    a = model.masks[sp["mask"]] if isinstance(sp["mask"], str) else sp["mask"]          # (a name, or the allow array itself)
    if sp["filt"] is None:
        return a
    col, kind, fs = model.case.filter_of(sp["filt"], nq)
    values, valid = model.cols[col]
    return np.stack([distinct_filter_ref.allowed(values, valid, kind, fs, q, a) for q in range(nq)])


def _of(a, q, n):
    if a is None:
        return np.ones(n, bool)
    return a[q] if a.ndim == 2 else a


def pick_radius(lo_hi, cuts_all=True):
    """a radius with hits for every query that cuts candidates for every query: between the largest per-query minimum and the
    smallest per-query maximum of the candidate distances.  cuts_all False (768 uniform dims: distances concentrate, every row is
    nearer to query 0, a centroid, than any row is to a uniform query, and no such radius exists): the same midpoint, which then
    leaves query 0 every candidate, the uniform queries none and the queries beside a corpus row some"""
    lo, hi = max(x[0] for x in lo_hi), min(x[1] for x in lo_hi)
    assert lo < hi or not cuts_all, (lo, hi)
    return float(np.float32((np.float64(lo) + np.float64(hi)) / 2))


def candidate_distances(oracle, model, sp, Q):
    """per query the output distances of its candidates (L2: d2, cosine: 0.5 d2, dot: -(q.x)), in candidate order"""
    out = []
    for q in Q:
        if sp["metric"] == "dot":
            cand = dot_ref.candidates(q, model.C, model.lists, sp["nprobe"])
            out.append(dot_ref.dist(q, model.X[cand.astype(np.int64)]))
            continue
        qv = cosine_ref.normalise(q) if sp["metric"] == "cos" else q
        cand = model.oidx(oracle, sp["metric"]).candidate_rows(qv, sp["nprobe"])
        d2 = l2_chain(model.rows_for(sp["metric"])[cand.astype(np.int64)], qv, REF4)
        out.append(cosine_ref.half(d2) if sp["metric"] == "cos" else d2)
    return out


def radius_for(oracle, model, sp, Q):
    """L2: compared with sqrt(d2) (sqrt_out); cosine and dot: with the output distance itself"""
    d = candidate_distances(oracle, model, sp, Q)
    if sp["metric"] == "l2":
        d = [np.sqrt(x) for x in d]
    return pick_radius([(float(x.min()), float(x.max())) for x in d if len(x)],          # (nprobe 1 on the emptied list: no candidates)
                       cuts_all=SHAPES[model.case.name].get("radius_cuts_all", True))


def _depth_probe(oracle, model, sp):
    """what a depth call's probe ranks: the metric's oracle index and the queries as it sees them (cosine: both normalised, as
    depth_ref.cosine_index_and_queries makes them)"""
    Q = model.case.queries(sp)
    return model.oidx(oracle, sp["metric"]), (cosine_ref.normalise(Q) if sp["metric"] == "cos" else Q)


def ratio_for(oracle, model, sp):
    """the d2_ratio of a RATIO depth spec: the float32 median, over the queries with d2_0 > 0, of d2_[(p0 + P) // 2] / d2_0 -- half
    of those queries then reach the middle rank and half do not (the distances come from depth_ref.probe_d2 on the oracle)"""
    oidx, Q = _depth_probe(oracle, model, sp)
    kc = int(oidx.n_clusters)
    p0, P = min(sp["nprobe"], kc), min(sp["maxp"], kc)
    assert p0 < P
    d2 = np.stack([depth_ref.probe_d2(oracle, oidx, q, P) for q in Q])
    ok = d2[:, 0] > 0
    assert ok.any() and d2.dtype == np.float32
    return float(np.float32(np.median(d2[ok, (p0 + P) // 2] / d2[ok, 0])))


def depth_used(oracle, model, sp):
    """uint32 [nq]: nprobe_used of a depth spec, from tests/depth_ref.py"""
    oidx, Q = _depth_probe(oracle, model, sp)
    if sp["depths"] is not None:
        assert len(sp["depths"]) == len(Q)
        return depth_ref.used_given(sp["depths"], sp["nprobe"], sp["maxp"], int(oidx.n_clusters))
    if not isinstance(sp["ratio"], float):
        raise ValueError("a ratio depth spec needs its ratio (resolve)")
    return depth_ref.used_ratio(oracle, oidx, Q, sp["ratio"], sp["nprobe"], sp["maxp"])


def _pad(rows, d, k):
    r = np.full(k, EMPTY, np.uint32)
    o = np.full(k, np.inf, np.float32)
    r[:len(rows)], o[:len(rows)] = rows, d
    return r, o


def _chains_agree(X, rows, qv):
    """the element-by-element chain and the 4-grouped chain of every one of `rows`, bit for bit"""
    x = X[rows.astype(np.int64)].reshape(len(rows), X.shape[1])
    return bool((l2_chain(x, qv, SEQ).view(np.uint32) == l2_chain(x, qv, REF4).view(np.uint32)).all())


def expect(oracle, model, sp):
    """The numpy answer of one call on one state -> dict of arrays (distances: d2 for L2, the output distance for cosine / dot; a
    range call's L2 distances are sqrt(d2))."""
    Q = model.case.queries(sp)
    nq, k, call, metric = len(Q), sp["k"], sp["call"], sp["metric"]
    allow = allowed_rows(model, sp, nq)
    X = model.rows_for(metric)
    out = {}

    def put(name, q, value):
        out.setdefault(name, []).append(value)

    if call == "range" and sp.get("radius") is None:
        raise ValueError("a range spec needs its radius (radius_for)")
    group = gvalid = None
    if call.startswith(("distinct", "grouped")):
        group, gvalid = model.cols["doc"]
    # the host forms of top-k follow the reference's heap where distances tie (pqv.h: the masked, keyed and expanding forms replay it
    # over the considered rows in arrival order); everything else orders by (d2, position)
    heap = call == "topk" and metric == "l2"
    depth = is_depth(sp)
    plain_heap = heap and allow is None and (depth or not sp["maxp"]) and not sp["maxc"]
    assert plain_heap == bool(sp["sqrt"])
    used_q = depth_used(oracle, model, sp) if depth else None
    if plain_heap and depth:
        # the host form "replays flagged queries through the reference heap over the query's first nprobe_used[q] lists": the
        # oracle's top-k at each distinct depth u, for the queries whose depth is u
        hrows, hdist = np.full((nq, k), EMPTY, np.uint32), np.full((nq, k), np.inf, np.float32)
        hnf, hnc = np.zeros(nq, np.uint32), np.zeros(nq, np.uint64)
        for u in sorted(set(used_q.tolist())):
            sel = used_q == u
            hrows[sel], hdist[sel], hnf[sel], hnc[sel] = model.oidx(oracle).topk_batch(X, Q[sel], k, u)
    elif plain_heap:
        hrows, hdist, hnf, hnc = model.oidx(oracle).topk_batch(X, Q, k, sp["nprobe"])
    lims = [0]
    for q in range(nq):
        qv = cosine_ref.normalise(Q[q]) if metric == "cos" else Q[q]
        a_q = _of(allow, q, model.n)
        if metric == "dot":
            kw = dict(max_candidates=sp["maxc"], allow=None if allow is None else a_q)
            if call == "range":
                r, d, w, c = dot_ref.range_ref(qv, model.C, model.lists, X, sp["radius"], sp["nprobe"], max_results=sp["maxr"], **kw)
                put("rows", q, r); put("d", q, d); put("nw", q, w); put("nc", q, c)
                lims.append(lims[-1] + len(r))
            else:
                r, d, f, c = dot_ref.topk_ref(qv, model.C, model.lists, X, k, sp["nprobe"], **kw)
                put("rows", q, r); put("d", q, d); put("nf", q, f); put("nc", q, c)
            continue
        oidx = model.oidx(oracle, metric)
        used = sp["nprobe"]
        if depth:
            used = int(used_q[q])
            put("used", q, used)
        elif sp["maxp"]:
            if group is None:
                used = expand_ref.nprobe_used(oidx, model.lists, a_q, qv, k, sp["nprobe"], sp["maxp"])
            else:
                used = distinct_expand_ref.nprobe_used(oidx, model.lists, group, gvalid, a_q, qv, k, sp["nprobe"], sp["maxp"])
            put("used", q, used)
        cand = oidx.candidate_rows(qv, used)
        put("nc", q, len(cand))
        if call == "range":
            if allow is None and metric == "l2":
                r, d, w, _ = range_oracle.range_query(cand, X, qv, sp["radius"], max_candidates=sp["maxc"], max_results=sp["maxr"])
            else:
                r, d, w, _ = mask_ref.masked_range(cand, a_q, X, qv, sp["radius"], max_candidates=sp["maxc"], max_results=sp["maxr"],
                                                   halve=metric == "cos")
            put("rows", q, r); put("d", q, d); put("nw", q, w)
            lims.append(lims[-1] + len(r))
        elif call.startswith("distinct"):
            r, d, g, _, _ = distinct_ref.distinct_topk(cand, group, gvalid, a_q, X, qv, k, max_candidates=sp["maxc"])
            rr, dd = _pad(r, d, k)
            gg = np.zeros(k, np.int64)
            gg[:len(g)] = g
            put("rows", q, rr); put("d", q, dd); put("grp", q, gg); put("nf", q, len(r))
        elif call.startswith("grouped"):
            r, d, g, c, f, _, _ = grouped_ref.grouped_topk(cand, group, gvalid, a_q, X, qv, k, sp["m"], max_candidates=sp["maxc"])
            put("rows", q, r); put("d", q, d); put("grp", q, g); put("grows", q, c); put("nf", q, f)
        else:
            if plain_heap:
                assert hnc[q] == len(cand)
                r, d = hrows[q, :hnf[q]], hdist[q, :hnf[q]]
                assert (np.sqrt(l2_chain(X[r.astype(np.int64)].reshape(len(r), model.dim), qv, REF4)).view(np.uint32) == d.view(np.uint32)).all()
            elif heap and model.case.integer and _chains_agree(X, mask_ref.considered(cand, a_q, sp["maxc"])[0], qv):
                # the heap over the considered rows: the oracle's is exec.rs' (the element-by-element chain), which on these small
                # integers is the 4-grouped chain bit for bit (every partial sum is an exact integer)
                r, d = oracle.topk_df(X, mask_ref.considered(cand, a_q, sp["maxc"])[0], qv, k)
                assert (d.view(np.uint32) == l2_chain(X[r.astype(np.int64)].reshape(len(r), model.dim), qv, REF4).view(np.uint32)).all()
            else:
                r, d, _, _ = mask_ref.masked_topk(cand, a_q, X, qv, k, max_candidates=sp["maxc"])
                if heap and model.case.integer:
                    # query 0, a centroid, is no vector of small integers: where its two chains round differently (long rows) the
                    # oracle's heap states nothing about the 4-grouped one.  Its k + 1 nearest considered rows are then all at
                    # different distances, and there the heap's order is (d2, position)
                    near = np.sort(l2_chain(X[mask_ref.considered(cand, a_q, sp["maxc"])[0].astype(np.int64)].reshape(-1, model.dim), qv, REF4))[:k + 1]
                    assert q == 0 and len(np.unique(near)) == len(near), (q, near)
                if sp["sqrt"]:
                    d = np.sqrt(d)
            if metric == "cos":
                d = cosine_ref.half(d)
            rr, dd = _pad(r, d, k)
            put("rows", q, rr); put("d", q, dd); put("nf", q, len(r))
    if call == "range":
        cat = lambda xs, t: np.concatenate(xs).astype(t) if xs else np.zeros(0, t)      # noqa: E731
        return {"lims": np.array(lims, np.uint64), "rows": cat(out["rows"], np.uint32), "d": cat(out["d"], np.float32),
                "nw": np.array(out["nw"], np.uint64), "nc": np.array(out["nc"], np.uint64)}
    res = {"rows": np.stack(out["rows"]).astype(np.uint32), "d": np.stack(out["d"]).astype(np.float32), "nf": np.array(out["nf"], np.uint32),
           "nc": np.array(out["nc"], np.uint64)}
    if "grp" in out:
        res["grp"] = np.stack(out["grp"]).astype(np.int64)
    if "grows" in out:
        res["grows"] = np.stack(out["grows"]).astype(np.uint32)
    if "used" in out:
        res["used"] = np.array(out["used"], np.uint32)
    return res


def passing_in(oracle, model, sp, nprobe):
    """per query the rows its filter passes among the candidates of `nprobe` lists"""
    Q = model.case.queries(sp)
    allow = allowed_rows(model, sp, len(Q))
    return np.array([int(_of(allow, q, model.n)[model.oidx(oracle).candidate_rows(Q[q], nprobe).astype(np.int64)].sum()) for q in range(len(Q))])


def same(got, want, skip=(), what=""):
    """every output of a call, bit for bit"""
    assert set(got) == set(want), (sorted(got), sorted(want))
    for name in want:
        if name in skip:
            continue
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {name}: {a.shape} {a.dtype} against {b.shape} {b.dtype}"
        bad = np.nonzero((a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1)).any(axis=1))[0] if a.ndim and len(a) else []
        assert len(bad) == 0, f"{what}: {name} differs at {list(bad[:8])}: got {a[bad[0]]}, want {b[bad[0]]}"


# ---- the calls every (case, state) is held to ---------------------------------------------------------------------------------------
def given_depths(nq, p0, P):
    """the given depths of a batch: below, at and above the floor p0 and the ceiling P, cycled (query 0 gets 0)"""
    vals = [0, 1, p0, (p0 + P) // 2, P, P + 1, 2 ** 32 - 1, p0 + 1]
    return np.array([vals[i % len(vals)] for i in range(nq)], np.uint32)


def modes(case_name):
    """name -> spec: what tests/test_gpu_mutated_search.py runs on every state of a case (int8_256: plain, per-query depths, cosine, masked and distinct)"""
    sh = SHAPES[case_name]
    nf, mp = sh["nprobe_f"], sh["max_nprobe"]
    full = case_name != "int8_256"
    m = {}
    for call in ("topk", "topk_device"):
        m[f"{call}"] = spec(call)
        m[f"{call}_k1"] = spec(call, k=1)
        m[f"{call}_k_above_one_list"] = spec(call, k=1024, nprobe=1)
        m[f"{call}_nq1"] = spec(call, nq=1)
        for cap, n in (("below", CAP), ("at", None), ("above", 1 << 20)):
            m[f"{call}_cap_{cap}"] = spec(call, maxc=n)               # "at": the first query's candidate count, filled in per state
        if call == "topk_device" or not sh["integer"]:
            # (pqv_topk's cosine is the d2-sorted heap of the normalised rows: where d2 ties, as on `ties`, no reference here states
            #  it -- the oracle's heaps sort by sqrt(d2) or run the element-by-element chain; the device form's (d2, position) stays)
            m[f"{call}_cosine"] = spec(call, metric="cos")
        m[f"{call}_masked"] = spec(call, mask="dense")
        m[f"{call}_masked_sparse"] = spec(call, mask="sparse", nprobe=nf)
    if not sh["integer"]:
        m["cosine_cap"] = spec("topk", metric="cos", maxc=CAP)
    m["masked_cap"] = spec("topk", mask="dense", maxc=CAP)
    m["distinct"] = spec("distinct")
    m["grouped"] = spec("grouped")
    m["distinct_device"] = spec("distinct_device")
    m["grouped_device"] = spec("grouped_device")
    m["distinct_masked"] = spec("distinct", mask="dense")
    if case_name == "screened":
        m["topk_160"] = spec("topk", q160=True)
        m["topk_device_160"] = spec("topk_device", q160=True)
        m["topk_masked_160"] = spec("topk", q160=True, mask="dense")
    # per-query probe depths (plain calls: int8_256 has them all).  Given: the cycle of `given_depths` -- query 0, the emptied
    # list's centroid, gets 0 and so walks nprobe_f lists --; ratio: ratio_for, filled in by resolve()
    dkw = dict(nprobe=nf, maxp=mp)
    m["depth_given"] = spec("topk", depths=given_depths(32, nf, mp), **dkw)
    m["depth_given_device"] = spec("topk_device", depths=given_depths(32, nf, mp), **dkw)
    m["depth_ratio"] = spec("topk", ratio=RESOLVE, **dkw)
    m["depth_ratio_device"] = spec("topk_device", ratio=RESOLVE, **dkw)
    m["depth_ratio_k1"] = spec("topk", k=1, ratio=RESOLVE, **dkw)
    # k above one list's rows: the answer of a query at depth 1 is every candidate
    m["depth_given_device_k1000"] = spec("topk_device", k=1000, nprobe=1, maxp=2, depths=np.array([1, 2] * 16, np.uint32))
    # one query: the uniform call is the fused probe with its own bucketing, the depth call goes through the general pair sort
    m["depth_given_device_nq1"] = spec("topk_device", nq=1, depths=np.array([(nf + mp) // 2], np.uint32), **dkw)
    if not sh["integer"]:          # (the host cosine form: as topk_cosine above)
        m["depth_ratio_cosine"] = spec("topk", metric="cos", ratio=RESOLVE, **dkw)
    m["depth_ratio_device_cosine"] = spec("topk_device", metric="cos", ratio=RESOLVE, **dkw)
    if case_name == "screened":
        m["depth_ratio_160"] = spec("topk", q160=True, ratio=RESOLVE, **dkw)
        m["depth_given_device_160"] = spec("topk_device", q160=True, depths=given_depths(160, nf, mp), **dkw)
    if not full:
        return m
    m["range"] = spec("range")
    m["range_masked"] = spec("range", mask="dense")
    m["range_max_results"] = spec("range", maxr=5)
    m["range_cap"] = spec("range", maxc=CAP)
    m["range_cosine"] = spec("range", metric="cos")
    m["range_masked_cap"] = spec("range", mask="dense", maxc=CAP, maxr=7)
    if case_name in ("exact30", "screened", "far768"):
        m["dot"] = spec("topk", metric="dot")
        m["dot_device"] = spec("topk_device", metric="dot")
        m["dot_range"] = spec("range", metric="dot")
        m["dot_masked"] = spec("topk", metric="dot", mask="dense")
        m["dot_range_masked"] = spec("range", metric="dot", mask="dense")
    for f in ("eq", "in", "range", "eq64"):
        m[f"keyed_{f}"] = spec("topk", filt=f, nprobe=nf)
        m[f"keyed_{f}_masked"] = spec("topk", filt=f, mask="dense", nprobe=nf)
        m[f"keyed_{f}_device"] = spec("topk_device", filt=f, nprobe=nf)
        m[f"range_keyed_{f}"] = spec("range", filt=f, nprobe=nf)
    m["keyed_eq_cap"] = spec("topk", filt="eq", nprobe=nf, maxc=CAP)
    m["expand_masked"] = spec("topk", mask="sparse", nprobe=nf, maxp=mp)
    m["expand_masked_device"] = spec("topk_device", mask="sparse", nprobe=nf, maxp=mp)
    for f in ("eq", "in", "range"):
        m[f"expand_{f}"] = spec("topk", filt=f, nprobe=nf, maxp=mp)
    m["expand_eq_masked"] = spec("topk", filt="eq", mask="dense", nprobe=nf, maxp=mp)
    m["expand_eq_device"] = spec("topk_device", filt="eq", nprobe=nf, maxp=mp)
    for call in ("distinct", "grouped"):
        m[f"{call}_filtered_eq"] = spec(call, filt="eq", nprobe=nf)
        m[f"{call}_filtered_range_masked"] = spec(call, filt="range", mask="dense", nprobe=nf)
        m[f"{call}_expand"] = spec(call, mask="sparse", nprobe=nf, maxp=mp)
        m[f"{call}_expand_eq"] = spec(call, filt="eq", nprobe=nf, maxp=mp)
        m[f"{call}_device_filtered_eq"] = spec(call + "_device", filt="eq", nprobe=nf)
        m[f"{call}_device_expand"] = spec(call + "_device", mask="sparse", nprobe=nf, maxp=mp)
    return m


def resolve(oracle, model, sp):
    """a spec with what depends on the state filled in: the cap "at" the candidate count, a range call's radius, a ratio depth
    call's ratio"""
    sp = dict(sp)
    if sp["ratio"] == RESOLVE:
        sp["ratio"] = ratio_for(oracle, model, sp)
    if sp["maxc"] is None:
        sp["maxc"] = len(model.oidx(oracle, sp["metric"]).candidate_rows(
            cosine_ref.normalise(model.case.Q[0]) if sp["metric"] == "cos" else model.case.Q[0], sp["nprobe"]))
    if sp["call"] == "range":
        sp["radius"] = radius_for(oracle, model, sp, model.case.queries(sp))
    return sp
