"""Range search over a key partition on the GPU (pqv_range_search_partition).

Every call is compared, bit for bit, against the numpy restatement (tests/partition_range_ref.py over
tests/partition_range_cases.py): rows, distance bits, lims, n_within and n_candidates.  The contract's equivalences are compared
call against call: (a) radius = +inf with max_results = k against topk_partition, ties included; (b) on the one-list index S1
against range_search(..., mask=M_q).  Radii come from the reference (prc.radii): below every distance, +inf, a median, and the
inclusive boundary at a considered row's own distance.  There are no tolerances."""
import ctypes as C

import numpy as np
import pytest

import key_filter_ref as kf
import partition_cases as pc
import partition_range_cases as prc
import partition_range_ref as prr
import partition_ref as pr
from test_gpu_partition import Setup, _host_filter, _same

pytestmark = pytest.mark.gpu

INF = np.float32(np.inf)
NAMES = ("lims", "rows", "dist", "n_within", "n_candidates")


def _same_range(got, exp, what=""):
    assert len(got) == 5
    for name, x, y in zip(NAMES, got, exp):
        x, y = np.asarray(x), np.asarray(y)
        assert x.dtype == y.dtype and x.shape == y.shape, f"{what}: {name} is {x.dtype}{x.shape}, expected {y.dtype}{y.shape}"
        assert (x.view(np.uint8) == y.view(np.uint8)).all(), f"{what}: {name} differs"


def search(s, part, queries, radius, flt, mask=None, metric=0, sqrt_out=False, max_results=0):
    return s.range_search_partition(queries, radius, part, mask=mask, max_results=max_results, metric=metric, sqrt_out=sqrt_out,
                                    **_host_filter(flt))


def check(s, part, case, ref_part, flt, radius, metric, allow=None, mask=None, sqrt_out=False, max_results=0, blocks=(0,), what=""):
    """the call under every `blocks` == the restatement"""
    exp = prc.reference(case, ref_part, flt, radius, sqrt_out, allow, max_results)
    for b in blocks:
        s.set_option("partition_blocks", b)
        got = search(s, part, case.queries, radius, flt, mask, metric, sqrt_out, max_results)
        _same_range(got, exp[:5], f"{what} {case.name} {flt[0]} radius={radius!r} sqrt_out={sqrt_out} max_results={max_results} blocks={b}")
    s.set_option("partition_blocks", 0)
    return got, exp


def check_radii(s, part, case, ref_part, flt, metric, allow=None, mask=None, sqrt_out=False, blocks=(0,), what="", distinct=True):
    """every derived radius of (case, filter, mask, scale); -> the hits seen, summed.  distinct: the case has no equal distances"""
    seen = 0
    for label, radius in prc.radii(prc.reference(case, ref_part, flt, INF, sqrt_out, allow)):
        got, _ = check(s, part, case, ref_part, flt, radius, metric, allow, mask, sqrt_out, blocks=blocks, what=f"{what} {label}")
        j = prc.boundary_j(label)
        if j is not None and distinct:
            assert got[3][0] == j + 1, "the boundary radius is inclusive and keeps nothing beyond it"
        seen += int(got[3].sum())
    return seen


@pytest.fixture(scope="module", params=list(pc.SHAPES))
def shape(request, pqv, oracle):
    return Setup(pqv, oracle, request.param)


@pytest.mark.parametrize("col", prc.COLUMNS)
def test_every_filter_radius_mask_and_scale(shape, col):
    """EQ (absent keys, keys outside i32 on the I32 column), RANGE (inverted, full) and IN (1 .. 1024 values, empty) x the derived
    radii x {no mask, a 50 % mask} x sqrt_out"""
    st, c = shape, shape.case
    allow = np.random.default_rng(3).random(c.n) < 0.5
    m = st.s.row_mask(allow)
    seen = 0
    try:
        for flt in c.filters(col):
            for al, mk in ((None, None), (allow, m)):
                for sqrt_out in (False, True):
                    seen += check_radii(st.s, st.parts[col], c, st.ref[col], flt, c.metric, al, mk, sqrt_out)
    finally:
        m.close()
    assert seen > 0


def test_partition_blocks_do_not_change_a_result(shape):
    st, c = shape, shape.case
    allow = np.random.default_rng(4).random(c.n) < 0.5
    m = st.s.row_mask(allow)
    try:
        for col in ("t3", "skew"):
            for flt in c.filters(col):
                for al, mk in ((None, None), (allow, m)):
                    check_radii(st.s, st.parts[col], c, st.ref[col], flt, c.metric, al, mk, True, blocks=prc.BLOCKS)
    finally:
        m.close()


def test_max_results_and_an_all_excluding_mask(shape):
    st, c = shape, shape.case
    none = st.s.row_mask(np.zeros(c.n, bool))
    try:
        for col in ("t3", "t64"):
            for flt in c.filters(col):
                for mr in (1, 3, 5000):
                    check(st.s, st.parts[col], c, st.ref[col], flt, INF, c.metric, max_results=mr)
                got, exp = check(st.s, st.parts[col], c, st.ref[col], flt, INF, c.metric, allow=np.zeros(c.n, bool), mask=none)
                assert got[0][-1] == 0 and (got[3] == 0).all() and (got[4] == prc.reference(c, st.ref[col], flt, INF)[4]).all()
    finally:
        none.close()


def test_seventy_queries(pqv, oracle):
    st = Setup(pqv, oracle, "1500x30", nq=70)
    c = st.case
    assert c.nq == 70
    for col in ("t3", "t64"):           # (t64's IN filter holds the 1024-value set)
        for flt in c.filters(col):
            check_radii(st.s, st.parts[col], c, st.ref[col], flt, c.metric, sqrt_out=True, blocks=prc.BLOCKS)


def test_piece_boundary(pqv):
    """one call of PARTITION_GRID_Q + 5 queries (32768: the grid's y, restated from csrc/api.cpp) on the smallest rows: 5 distinct
    queries and filters, cycled, so the reference is computed for 5 and tiled.  32768 is no multiple of 5: the queries past the
    boundary continue the cycle at its fourth pattern, so each of them has another IN set than the query 32768 places ahead of it --
    a second piece that kept the first one's filter slice or lims would answer for other keys.  The radius is the 75th smallest of
    the 1500 distances: about 15 rows a query ahead of the filter, at most 15 hits.  Every output is compared whole, and its part past the boundary on its own."""
    piece, n, dim = 32768, 300, 8
    nq = piece + 5
    rng = np.random.default_rng(77)
    data, q5 = rng.random((n, dim), dtype=np.float32), rng.random((5, dim), dtype=np.float32)
    tenant = rng.integers(0, 3, n).astype(np.int32)
    corpus = pqv.Corpus.upload(data)
    lists = [np.arange(i, n, 2, dtype=np.uint32) for i in range(2)]
    s = pqv.Searcher(pqv.Index.from_parts(dim, np.zeros((2, dim), np.float32), lists), corpus)
    part = s.key_partition(pqv.Column.upload(tenant))
    prows, pkeys = pr.build(tenant, None, np.arange(n))
    d5 = pr.distances("l2", pr.REF4, data, q5)
    radius = np.sort(d5.ravel())[5 * 15 - 1]
    reps = (nq + 4) // 5
    tile = lambda x: np.concatenate([x] * reps)[:nq]        # noqa: E731
    queries = tile(q5)
    sets5 = [[0], [1, 2], [], [0, 2, 5], [2]]
    assert all(sets5[(piece + i) % 5] != sets5[i] for i in range(5))
    lims5, vals5 = kf.sets_to_csr(sets5)
    lims, vals = kf.sets_to_csr((sets5 * reps)[:nq])
    for f5, f in ((("eq", kf.EQ, [0, 1, 2, 7, 1], None), ("eq", kf.EQ, ([0, 1, 2, 7, 1] * reps)[:nq], None)),
                  (("range", kf.RANGE, [0, 1, 2, 0, 1], [1, 2, 0, 2, 1]), ("range", kf.RANGE, ([0, 1, 2, 0, 1] * reps)[:nq], ([1, 2, 0, 2, 1] * reps)[:nq])),
                  (("in", kf.IN, [int(x) for x in lims5], [int(x) for x in vals5]), ("in", kf.IN, [int(x) for x in lims], [int(x) for x in vals]))):
        res5 = [prr.range_query(prows, pkeys, f5[1], f5[2], f5[3], q, d5[q], radius) for q in range(5)]
        assert max(r[2] for r in res5) <= 15
        exp_lims = np.zeros(nq + 1, np.uint64)
        exp_lims[1:] = np.cumsum(tile(np.array([len(r[0]) for r in res5], np.uint64)))
        exp = (exp_lims, np.concatenate([res5[i % 5][0] for i in range(nq)]), np.concatenate([res5[i % 5][1] for i in range(nq)]),
               tile(np.array([r[2] for r in res5], np.uint64)), tile(np.array([r[3] for r in res5], np.uint64)))
        got = search(s, part, queries, radius, f)
        _same_range(got, exp, f"{f[0]}: {nq} queries in one call")
        lo = int(exp_lims[piece])
        assert int(exp_lims[nq]) > lo, "the part past the boundary is not empty"
        _same_range((got[0][piece:] - got[0][piece], got[1][int(got[0][piece]):], got[2][int(got[0][piece]):], got[3][piece:], got[4][piece:]),
                    (exp_lims[piece:] - exp_lims[piece], exp[1][lo:], exp[2][lo:], exp[3][piece:], exp[4][piece:]),
                    f"{f[0]}: past the piece boundary")


def _groups(n_cand, budget):
    """the documented cut: consecutive queries while 12 B x the sum of their candidate counts fits `budget`; never empty"""
    groups, g0 = [], 0
    while g0 < len(n_cand):
        g1, entries = g0, 0
        while g1 < len(n_cand) and (g1 == g0 or (entries + int(n_cand[g1])) * 12 <= budget):
            entries += int(n_cand[g1])
            g1 += 1
        groups.append((g0, g1, entries))
        g0 = g1
    return groups


def test_the_group_cut_does_not_change_a_result(pqv, oracle):
    """partition_range_bytes small: the piece runs in several groups, one query's segment exceeds the budget alone.  The split
    is asserted through kernel_launches: the span launch, and per group with a candidate the range kernel and -- every segment
    is within one block's sort here -- one sort launch where the group has a hit."""
    st = Setup(pqv, oracle, "1500x30", nq=70)
    c = st.case
    for col, fi in (("t3", 1), ("t64", 2), ("skew", 0)):
        flt = c.filters(col)[fi]
        exp = prc.reference(c, st.ref[col], flt, INF)
        nc, nw = exp[4], exp[3]
        budget = 12 * int(np.sort(nc)[-1] - 1) if col == "skew" else 12 * int(nc.max()) * 2
        groups = _groups(nc, budget)
        assert len(groups) >= 3 and (col != "skew" or any(e * 12 > budget for _, _, e in groups)), "one query exceeds the budget alone"
        want = 1 + sum(int(e > 0) + int(nw[g0:g1].sum() > 0) for g0, g1, e in groups)
        one = 1 + int(nc.sum() > 0) + int(nw.sum() > 0)
        assert want > one
        for bytes_, launches in ((0, one), (budget, want)):
            st.s.set_option("partition_range_bytes", bytes_)
            before = st.s.counters()["kernel_launches"]
            _same_range(search(st.s, st.parts[col], c.queries, INF, flt, metric=c.metric), exp[:5], f"{col} budget {bytes_}")
            assert st.s.counters()["kernel_launches"] - before == launches, (col, bytes_)
        for label, radius in prc.radii(exp):
            check(st.s, st.parts[col], c, st.ref[col], flt, radius, c.metric, what=f"budget {budget} {label}")
        st.s.set_option("partition_range_bytes", 0)


def _topk_equivalence(s, part, queries, flt, metric, ks, mask=None, what=""):
    for k in ks:
        for sqrt_out in (False, True):
            lims, rows, dist, nw, nc = search(s, part, queries, INF, flt, mask, metric, sqrt_out, max_results=k)
            tr, td, tnf, tnc = s.topk_partition(queries, k, part, mask=mask, metric=metric, sqrt_out=sqrt_out, **_host_filter(flt))
            _same((np.diff(lims.astype(np.int64)).astype(np.uint32), nc), (tnf, tnc), f"{what} {flt[0]} k={k}: counts")
            for q in range(len(queries)):
                lo, hi = int(lims[q]), int(lims[q + 1])
                _same((rows[lo:hi], dist[lo:hi]), (tr[q, :tnf[q]], td[q, :tnf[q]]), f"{what} {flt[0]} k={k} query {q} vs topk_partition")


def test_infinite_radius_is_topk_partition(shape):
    """equivalence (a)"""
    st, c = shape, shape.case
    m = st.s.row_mask(np.random.default_rng(5).random(c.n) < 0.5)
    try:
        for col in ("t3", "t64"):
            for flt in c.filters(col):
                _topk_equivalence(st.s, st.parts[col], c.queries, flt, c.metric, (1, 10, 300, 1024), what=c.name)
            _topk_equivalence(st.s, st.parts[col], c.queries, c.filters(col)[1], c.metric, (10, 300), mask=m, what=c.name + " masked")
    finally:
        m.close()


def _tie_searcher(pqv, c):
    corpus = pqv.Corpus.upload(c.data)
    s = pqv.Searcher(pqv.Index.from_parts(c.dim, np.zeros((len(c.lists), c.dim), np.float32), c.lists), corpus)
    return s, s.key_partition(pqv.Column.upload(c.keys))


def test_ties_follow_distance_then_position(pqv):
    c = prc.TieCase()
    s, part = _tie_searcher(pqv, c)
    ref_part = c.partition()
    assert any(len(np.unique(row)) < len(row) // 4 for row in c.d), "the case is about equal distances"
    for flt in c.filters():
        _topk_equivalence(s, part, c.queries, flt, 0, (1, 10, 300, 1024), what="ties")
        for sqrt_out in (False, True):
            check_radii(s, part, c, ref_part, flt, 0, sqrt_out=sqrt_out, blocks=prc.BLOCKS, what="ties", distinct=False)
        check(s, part, c, ref_part, flt, INF, 0, max_results=100, blocks=prc.BLOCKS, what="ties")


@pytest.mark.parametrize("name", ["4096x128", "1500x30"])
def test_equals_the_masked_range_search_on_the_one_list_index(pqv, oracle, name):
    """equivalence (b): range_search(..., mask=M_q) on S1 with nprobe = 1, per query (aligned rows, and unaligned with a tail)"""
    st = Setup(pqv, oracle, name)
    c = st.case
    shared = np.random.default_rng(6).random(c.n) < 0.5
    m = st.s.row_mask(shared)
    try:
        for col in ("t3", "t64"):
            values, valid = c.columns[col]
            for flt in c.filters(col):
                for allow, mask, sqrt_out in ((None, None, True), (shared, m, False)):
                    rad = dict(prc.radii(prc.reference(c, st.ref[col], flt, INF, sqrt_out, allow)))
                    for label in ("inf", "median"):
                        if label not in rad:
                            continue
                        lims, rows, dist, nw, nc = search(st.s, st.parts[col], c.queries, rad[label], flt, mask, c.metric, sqrt_out, max_results=50)
                        for q in range(c.nq):
                            mq = st.s1.row_mask(kf.allowed_for(values, valid, flt[1], flt[2], flt[3], q, allow))
                            l1, r1, d1, w1, _ = st.s1.range_search(c.queries[q:q + 1], rad[label], 1, max_results=50, metric=c.metric,
                                                                   sqrt_out=sqrt_out, mask=mq)
                            mq.close()
                            lo, hi = int(lims[q]), int(lims[q + 1])
                            _same((rows[lo:hi], dist[lo:hi], nw[q:q + 1]), (r1, d1, w1), f"{name} {col} {flt[0]} {label} query {q} vs S1")
    finally:
        m.close()


def test_long_segments(pqv):
    """BIG: more than 8192 hits (two merge passes), under the mask more than 4096 (one), max_results inside the segment, and a
    finite radius in the middle of equal distances"""
    c = prc.BigCase()
    s, part = _tie_searcher(pqv, c)
    ref_part = c.partition()
    m = s.row_mask(c.shared)
    try:
        for flt in c.filters():
            got, _ = check(s, part, c, ref_part, flt, INF, 0, blocks=prc.BLOCKS, what="big")
            assert got[3].max() > 2 * prc.RANGE_SMALL
            got, _ = check(s, part, c, ref_part, flt, INF, 0, allow=c.shared, mask=m, sqrt_out=True, what="big masked")
            assert prc.RANGE_SMALL < got[3].max() <= 2 * prc.RANGE_SMALL
            for mr in prc.BIG_MAX_RESULTS:
                check(s, part, c, ref_part, flt, INF, 0, max_results=mr, what="big")
            check_radii(s, part, c, ref_part, flt, 0, sqrt_out=True, what="big", distinct=False)
        # the groups of a small budget run the long-segment path one after the other
        s.set_option("partition_range_bytes", 12 * 9500)
        for flt in c.filters():
            check(s, part, c, ref_part, flt, INF, 0, max_results=4097, what="big in groups")
        s.set_option("partition_range_bytes", 0)
    finally:
        m.close()


@pytest.mark.parametrize("name", prc.LONG_SHAPES)
def test_long_rows_cosine_and_dot(pqv, oracle, name):
    """multi-chunk rows, zero-padded storage ("260"), PQV_COSINE through the cosine layout and PQV_DOT (negative radii)"""
    c = prc.LongCase(name, oracle)
    lc = c.lc
    metric = {"l2": lc.metric, "cos": pqv.PQV_COSINE, "dot": pqv.PQV_DOT}[lc.kind]
    corpus = pqv.Corpus.upload(lc.data)
    s = pqv.Searcher(pqv.Index.from_parts(lc.dim, lc.centroids, lc.lists), corpus)
    m = s.row_mask(c.shared)
    seen = 0
    for col, (values, valid) in c.columns.items():
        part, ref_part = s.key_partition(pqv.Column.upload(values, valid)), c.partition(col)
        for flt in c.filters(col):
            for allow, mask in ((None, None), (c.shared, m)):
                for sqrt_out in (False, True):
                    seen += check_radii(s, part, c, ref_part, flt, metric, allow, mask, sqrt_out, blocks=prc.BLOCKS, what=name)
            _topk_equivalence(s, part, c.queries, flt, metric, (10, 300), what=name)
    m.close()
    assert seen > 1000


@pytest.mark.parametrize("name", ["4096x128", "1500x30"])
def test_removed_rows_are_in_no_hit(pqv, oracle, name):
    n = pc.SHAPES[name]["n"]
    removed = np.unique(np.random.default_rng(8).integers(0, n, n // 5))
    st = Setup(pqv, oracle, name, removed=removed)
    c = st.case
    for col in c.columns:
        for flt in c.filters(col):
            got, _ = check(st.s, st.parts[col], c, st.ref[col], flt, INF, c.metric, sqrt_out=True, blocks=(1, 0), what="removed")
            assert not np.isin(got[1], removed).any()
            check_radii(st.s, st.parts[col], c, st.ref[col], flt, c.metric, what="removed")


def test_counters_and_the_same_call_twice(shape):
    st, c = shape, shape.case
    flt = c.filters("t64")[2]
    m = st.s.row_mask(np.random.default_rng(5).random(c.n) < 0.25)
    try:
        for mask, allow in ((None, None), (m, m.to_bytes().astype(bool))):
            exp = prc.reference(c, st.ref["t64"], flt, INF, allow=allow)
            radius = prc.radii(exp)[2][1]
            exp = prc.reference(c, st.ref["t64"], flt, radius, allow=allow)
            before = st.s.counters()
            a = search(st.s, st.parts["t64"], c.queries, radius, flt, mask, c.metric)
            mid = st.s.counters()
            b = search(st.s, st.parts["t64"], c.queries, radius, flt, mask, c.metric)
            _same_range(a, exp[:5], "the first call")
            _same_range(b, a, "the same call twice")
            after = st.s.counters()
            for lo, hi in ((before, mid), (mid, after)):
                assert hi["queries"] - lo["queries"] == c.nq
                assert hi["candidate_rows"] - lo["candidate_rows"] == int(exp[4].sum())
                assert hi["embeddings_fetched"] - lo["embeddings_fetched"] == exp[5]
                assert hi["screened_pairs"] == lo["screened_pairs"] and hi["screen_survivors"] == lo["screen_survivors"]
                assert hi["exact_replays"] == lo["exact_replays"]
    finally:
        m.close()


def test_timing_sees_the_distance_pass(shape):
    st, c = shape, shape.case
    st.s.set_timing(True)
    try:
        st.s.timing_read()
        search(st.s, st.parts["t3"], c.queries, INF, c.filters("t3")[1], metric=c.metric)
        rerank, total, calls = st.s.timing_read()
        assert calls == 1 and 0 < rerank <= total
        search(st.s, st.parts["t3"], c.queries, INF, ("eq", kf.EQ, [3] * c.nq, None), metric=c.metric)      # (no candidate: nothing runs)
        assert st.s.timing_read()[2] == 1
    finally:
        st.s.set_timing(False)


def test_empty_batches_refusals_and_null_outputs(pqv, oracle):
    c = pc.Case("1500x30")
    built = oracle.build_index(c.data, n_clusters=c.kc, max_iters=5, workers=1)
    corpus = pqv.Corpus.upload(c.data)
    index = pqv.Index.from_parts(c.dim, built.centroids, [np.asarray(l, np.uint32) for l in built.lists()])
    s, other = pqv.Searcher(index, corpus), pqv.Searcher(index, corpus)
    part = s.key_partition(pqv.Column.upload(*c.columns["t64"]))
    flt = c.filters("t64")[0]
    # nq = 0: lims is allocated and holds [0]
    lims, rows, dist, nw, nc = s.range_search_partition(c.queries[:0], 1.0, part, query_keys=[])
    assert lims.tolist() == [0] and len(rows) == len(dist) == len(nw) == len(nc) == 0
    with pytest.raises(pqv.PqvError, match="key partition belongs to another searcher"):
        other.range_search_partition(c.queries, 1.0, part, query_keys=flt[2])
    om = other.row_mask(np.ones(c.n, bool))
    with pytest.raises(pqv.PqvError, match="row mask belongs to another searcher"):
        s.range_search_partition(c.queries, 1.0, part, query_keys=flt[2], mask=om, metric=9)       # (ahead of the metric)
    om.close()
    with pytest.raises(pqv.PqvError, match="unknown metric"):
        s.range_search_partition(c.queries[:, :29], 1.0, part, query_keys=flt[2], metric=9)         # (ahead of the query length)
    with pytest.raises(pqv.PqvError, match="Query dimension mismatch: expected 30, got 29"):
        s.range_search_partition(c.queries[:, :29], 1.0, part, query_keys=flt[2])
    # behind the wrapper's own checks: the library's, in the contract's order
    lib, ffi = pqv._ffi.lib(), pqv._ffi
    qk = (C.c_int64 * c.nq)(*flt[2])
    f = ffi.KeyFilter(ffi.PQV_KEY_EQ, 0, C.cast(qk, C.c_void_p), None)
    q = np.ascontiguousarray(c.queries)
    lp, rp, dp = ffi.u64p(), ffi.u32p(), ffi.f32p()

    def raw(radius, qptr=q.ctypes.data_as(ffi.f32p), qlen=c.dim, out=(C.byref(lp), C.byref(rp), C.byref(dp)), nw=None, nc=None):
        return lib.pqv_range_search_partition(s._h, part._h, C.byref(f), None, qptr, c.nq, qlen, radius, 0, 0, 0, *out, nw, nc)

    for kw, text in ((dict(radius=float("nan"), qlen=29), b"Query dimension mismatch"),
                     (dict(radius=float("nan"), out=(None, None, None)), b"radius must not be NaN"),
                     (dict(radius=1.0, qptr=None, out=(C.byref(lp), None, C.byref(dp))), b"lims/row_idx/dist must not be NULL"),
                     (dict(radius=1.0, qptr=None), b"queries must not be NULL")):
        rc = raw(**kw)
        assert rc == ffi.PQV_ERR_INVALID and text in lib.pqv_last_error(), (rc, lib.pqv_last_error())
    # n_within and n_candidates may be NULL
    assert raw(float("inf")) == 0
    exp = prc.reference(c, c.partition("t64"), flt, INF)
    got = np.ctypeslib.as_array(lp, shape=(c.nq + 1,)).copy()
    lib.pqv_range_free(lp, rp, dp)
    assert (got == exp[0]).all() and got[-1] > 0
    # a column of NULLs only: an empty partition answers nothing
    empty = s.key_partition(pqv.Column.upload(np.zeros(c.n, np.int64), np.zeros(c.n, np.uint8)))
    lims, rows, dist, nw, nc = s.range_search_partition(c.queries, INF, empty, query_keys=[0] * c.nq)
    assert (lims == 0).all() and len(rows) == 0 and (nw == 0).all() and (nc == 0).all()
    for h in (empty, part, s, other):
        h.close()
