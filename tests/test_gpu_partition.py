"""Key partitions on the GPU (pqv_key_partition_create, pqv_topk_partition, pqv_topk_partition_device).

Every call is compared, bit for bit, against the numpy restatement (tests/partition_ref.py over tests/partition_cases.py) AND
against the existing filtered call on S1 -- a searcher over Index.from_parts(dim, one centroid, [all indexed rows ascending]) on
the same corpus, nprobe = 1, max_candidates = 0 -- per the contract's equivalence; PQV_DOT, which the keyed calls refuse, against
pqv_topk_masked_device on S1 per query under the mask M_q.  The inputs have no two rows equally far from a query
(partition_cases), so RANGE and IN qualify for the S1 comparison too; the one case with deliberate ties is held to the
restatement's (distance, position) order.  There are no tolerances."""
import numpy as np
import pytest

import key_filter_ref as kf
import long_rows_cases as lrc
import partition_cases as pc
import partition_ref as pr

pytestmark = pytest.mark.gpu

EMPTY = 0xFFFFFFFF


def _same(got, exp, what=""):
    for i, (x, y) in enumerate(zip(got, exp)):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and (x.view(np.uint8) == y.view(np.uint8)).all(), f"{what}: output {i} differs"


def _dev():
    import torch
    return torch.device("cuda", 0)


def _i64_tensor(v):
    import torch
    return torch.tensor([int(x) for x in v] or [0], dtype=torch.int64, device=_dev())


def _device_filter(flt):
    """the filter's device arrays as the device entry points' keywords -> (keywords, the tensors to keep alive)"""
    _, kind, a, b = flt
    if kind == kf.EQ:
        t = (_i64_tensor(a),)
        return dict(query_keys=t[0].data_ptr()), t
    if kind == kf.RANGE:
        t = (_i64_tensor(a), _i64_tensor(b))
        return dict(query_key_ranges=(t[0].data_ptr(), t[1].data_ptr())), t
    t = (_i64_tensor(a), _i64_tensor(b))            # (lims are below 2^63: the same bits as u64)
    return dict(query_key_sets=(t[0].data_ptr(), t[1].data_ptr())), t


def _host_filter(flt):
    _, kind, a, b = flt
    if kind == kf.EQ:
        return dict(query_keys=a)
    if kind == kf.RANGE:
        return dict(query_key_ranges=(a, b))
    return dict(query_key_sets=[b[a[i]:a[i + 1]] for i in range(len(a) - 1)])


def _outputs(nq, k):
    import torch
    dev = _dev()
    return (torch.full((nq, k), 7, dtype=torch.int32, device=dev), torch.full((nq, k), -1.0, dtype=torch.float32, device=dev),
            torch.full((nq,), 7, dtype=torch.int32, device=dev), torch.full((nq,), 7, dtype=torch.int64, device=dev))


def _results(r_t, d_t, nf_t, nc_t):
    return (r_t.cpu().numpy().view(np.uint32), d_t.cpu().numpy(), nf_t.cpu().numpy().astype(np.uint32), nc_t.cpu().numpy().astype(np.uint64))


def part_device(s, part, q, k, flt, mask=None, metric=0, sqrt_out=False):
    """topk_partition_device -> (rows, dist, n_found, n_candidates)"""
    import torch
    q_t = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(_dev())
    out = _outputs(len(q), k)
    kw, alive = _device_filter(flt)
    torch.cuda.synchronize()
    s.topk_partition_device(q_t.data_ptr(), len(q), k, part, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(),
                            mask=mask, metric=metric, sqrt_out=sqrt_out, **kw)
    torch.cuda.synchronize()
    del alive
    return _results(*out)


def s1_device(s1, q, k, keys=None, flt=None, mask=None, metric=0, sqrt_out=False):
    """topk_device on S1 with nprobe = 1 -> (rows, dist, n_found)"""
    import torch
    q_t = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(_dev())
    out = _outputs(len(q), k)
    kw, alive = _device_filter(flt) if flt is not None else ({}, ())
    if keys is not None:
        kw["keys"] = keys
    if mask is not None:
        kw["mask"] = mask
    torch.cuda.synchronize()
    s1.topk_device(q_t.data_ptr(), len(q), k, 1, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), metric=metric,
                   sqrt_out=sqrt_out, **kw)
    torch.cuda.synchronize()
    del alive
    return _results(*out)[:3]


def one_list(pqv, dim, corpus, indexed, flags=0):
    """S1 of the contract: one list = all indexed rows ascending, any centroid"""
    rows = np.sort(np.asarray(indexed)).astype(np.uint32)
    return pqv.Searcher(pqv.Index.from_parts(dim, np.zeros((1, dim), np.float32), [rows]), corpus, flags)


class Setup:
    """A shape's case on the device: the corpus, an oracle-built index and its searcher, S1, and per key column the resident
    column, the partition, S1's row keys and the restatement's partition."""

    def __init__(self, pqv, oracle, name, nq=5, flags=0, removed=None):
        self.pqv = pqv
        self.case = c = pc.Case(name, nq)
        built = oracle.build_index(c.data, n_clusters=c.kc, max_iters=5, workers=1)
        self.corpus = pqv.Corpus.upload(c.data)
        index = pqv.Index.from_parts(c.dim, built.centroids, [np.asarray(l, np.uint32) for l in built.lists()])
        self.indexed = np.arange(c.n)
        if removed is not None:
            index = index.remove(rows=removed)
            self.indexed = np.setdiff1d(self.indexed, removed)
        s1_corpus = self.corpus
        if flags & pqv.PQV_RELEASE_ROW_ORDER:      # (the searcher takes the corpus' rows with it: S1 reads a copy of its own)
            s1_corpus = self.s1_corpus = pqv.Corpus.upload(c.data)
        self.s1 = one_list(pqv, c.dim, s1_corpus, self.indexed)
        self.s = pqv.Searcher(index, self.corpus, flags)
        self.cols, self.parts, self.keys1, self.ref = {}, {}, {}, {}
        for col, (values, valid) in c.columns.items():
            self.cols[col] = pqv.Column.upload(values, valid)
            self.parts[col] = self.s.key_partition(self.cols[col])
            self.keys1[col] = self.s1.row_keys(self.cols[col])
            self.ref[col] = c.partition(col, self.indexed)

    def check(self, col, flt, k, allow=None, mask=None, mask1=None, sqrt_out=False, blocks=(0,), what=""):
        """the device form under every `blocks` == the restatement == the filtered call on S1"""
        c = self.case
        exp = c.topk(self.ref[col], flt, k, sqrt_out=sqrt_out, allow=allow)
        for b in blocks:
            self.s.set_option("partition_blocks", b)
            got = part_device(self.s, self.parts[col], c.queries, k, flt, mask=mask, metric=c.metric, sqrt_out=sqrt_out)
            _same(got, exp[:4], f"{what} {col} {flt[0]} k={k} blocks={b} vs the restatement")
        self.s.set_option("partition_blocks", 0)
        twin = s1_device(self.s1, c.queries, k, keys=self.keys1[col], flt=flt, mask=mask1, metric=c.metric, sqrt_out=sqrt_out)
        _same(got[:3], twin, f"{what} {col} {flt[0]} k={k} vs the filtered call on S1")
        return got


@pytest.fixture(scope="module", params=list(pc.SHAPES))
def shape(request, pqv, oracle):
    return Setup(pqv, oracle, request.param)


def test_partition_build_equals_numpy(shape):
    st = shape
    for col, (values, valid) in st.case.columns.items():
        part, (prows, pkeys) = st.parts[col], st.ref[col]
        v, cnt = pr.distinct(pkeys)
        assert part.rows == len(prows) and part.n_keys == len(v), col
        assert part.dtype == (st.pqv._ffi.PQV_COL_I32 if values.dtype == np.int32 else st.pqv._ffi.PQV_COL_I64)
        gv, gc = part.keys()
        assert gv.dtype == np.int64 and gc.dtype == np.uint64
        _same((gv, gc), (v, cnt), f"keys() of {col}")
        gv, gc = part.keys(3)
        _same((gv, gc), (v[:3], cnt[:3]), f"keys(3) of {col}")
        assert int(gc.sum()) <= part.rows


@pytest.mark.parametrize("col", ["t3", "t64", "distinct", "skew"])
def test_every_filter_k_and_block_count(shape, col):
    """EQ, RANGE (a > b, the full range, beyond i32) and IN (1, 5, 1024 values, absent ones, empty) at k in {1, 10, 100, 300, 1024};
    partition_blocks in {1, 3, by rule} at k = 10 and 300.  Absent keys, keys outside i32 on the I32 columns and keys with fewer
    than k rows give n_found < k, EMPTY / +inf behind it."""
    st = shape
    for flt in st.case.filters(col):
        for k in pc.KS:
            got = st.check(col, flt, k, blocks=pc.BLOCKS if k in (10, 300) else (0,))
            rows, dist, nf, nc = got
            assert (nf <= np.minimum(k, nc)).all()
            for q in range(st.case.nq):
                assert (rows[q, nf[q]:] == EMPTY).all() and np.isposinf(dist[q, nf[q]:]).all()
    if col == "t64":
        assert (st.check(col, st.case.filters(col)[0], 100)[2][:3] < 100).all(), "keys with fewer than k rows"


def test_full_range_is_the_unmasked_call_on_s1(shape):
    st, c = shape, shape.case
    for col in ("t3", "skew"):                     # (no NULLs: every indexed row has a key)
        flt = ("range", kf.RANGE, [kf.INT64_MIN] * c.nq, [kf.INT64_MAX] * c.nq)
        for k in (10, 300):
            got = st.check(col, flt, k)
            assert (got[3] == len(st.indexed)).all()
            _same(got[:3], s1_device(st.s1, c.queries, k, metric=c.metric), f"{col} k={k} vs pqv_topk_device on S1")


def test_host_form_equals_device_form(shape):
    st, c = shape, shape.case
    for col in ("t64", "skew"):
        for flt in c.filters(col):
            for k, sqrt_out in ((10, True), (300, False)):
                dev = part_device(st.s, st.parts[col], c.queries, k, flt, metric=c.metric, sqrt_out=sqrt_out)
                host = st.s.topk_partition(c.queries, k, st.parts[col], metric=c.metric, sqrt_out=sqrt_out, **_host_filter(flt))
                _same(host, dev, f"{col} {flt[0]} k={k}")
                _same(host, c.topk(st.ref[col], flt, k, sqrt_out=sqrt_out)[:4], f"{col} {flt[0]} k={k} sqrt_out={sqrt_out}")


def test_shared_mask(shape):
    """a mask allows about half the rows, and one allows none: considered rows keep their unmasked positions, n_candidates is
    taken before the mask"""
    st, c = shape, shape.case
    for allow in (np.random.default_rng(3).random(c.n) < 0.5, np.zeros(c.n, bool)):
        m, m1 = st.s.row_mask(allow), st.s1.row_mask(allow)
        try:
            for col in ("t3", "distinct"):
                for flt in c.filters(col):
                    for k in (10, 300):
                        got = st.check(col, flt, k, allow=allow, mask=m, mask1=m1, blocks=pc.BLOCKS, what="masked")
                        _same(got[3:], c.topk(st.ref[col], flt, k)[3:4], "n_candidates")
                        if not allow.any():
                            assert (got[2] == 0).all()
                host = st.s.topk_partition(c.queries, 10, st.parts["t3"], mask=m, metric=c.metric, **_host_filter(c.filters("t3")[1]))
                _same(host, c.topk(st.ref["t3"], c.filters("t3")[1], 10, sqrt_out=True, allow=allow)[:4], "host form under a mask")
        finally:
            m.close()
            m1.close()


def test_same_call_twice_and_counters(shape):
    st, c = shape, shape.case
    flt = c.filters("t64")[2]
    m = st.s.row_mask(np.random.default_rng(5).random(c.n) < 0.25)
    try:
        for mask, allow in ((None, None), (m, m.to_bytes().astype(bool))):
            exp = c.topk(st.ref["t64"], flt, 10, allow=allow)
            before = st.s.counters()
            a = part_device(st.s, st.parts["t64"], c.queries, 10, flt, mask=mask, metric=c.metric)
            mid = st.s.counters()
            b = part_device(st.s, st.parts["t64"], c.queries, 10, flt, mask=mask, metric=c.metric)
            _same(a, b, "the same call twice")
            h = st.s.topk_partition(c.queries, 10, st.parts["t64"], mask=mask, metric=c.metric, sqrt_out=False, **_host_filter(flt))
            _same(h, a, "host form")
            after = st.s.counters()
            for lo, hi, calls in ((before, mid, 1), (mid, after, 2)):
                assert hi["queries"] - lo["queries"] == calls * c.nq
                assert hi["candidate_rows"] - lo["candidate_rows"] == calls * int(exp[3].sum())
                assert hi["embeddings_fetched"] - lo["embeddings_fetched"] == calls * exp[4]
                assert hi["screened_pairs"] == lo["screened_pairs"] and hi["screen_survivors"] == lo["screen_survivors"]
                assert hi["exact_replays"] == lo["exact_replays"]
    finally:
        m.close()


def test_masked_flush_edges(pqv, oracle):
    """The masked walk's last tile, with one block per query (wave w takes the windows 4 t + w) over a run of about 1365 positions:
    the mask allows exactly the rows at the run's sequence positions (i) 0 .. 63 -- wave 0 emits one full tile and flushes nothing;
    (ii) 0 .. 63 and 256 -- wave 0's second window leaves one queued; (iii) 0 alone; (iv) 64 .. 126 -- 63 rows, all in wave 1."""
    st = Setup(pqv, oracle, "4096x128")
    c, k = st.case, 10
    flt = ("eq", kf.EQ, [7] * c.nq, None)
    prows, pkeys = st.ref["t3"]
    run = prows[pr.sequence(pkeys, kf.EQ, flt[2], None, 0)]          # the rows at the sequence's positions
    assert 1200 < len(run) < 1500
    st.s.set_option("partition_blocks", 1)
    try:
        for label, positions, n_found in (("i", range(64), 10), ("ii", [*range(64), 256], 10), ("iii", [0], 1), ("iv", range(64, 127), 10)):
            allow = np.zeros(c.n, bool)
            allow[run[list(positions)]] = True
            assert allow.sum() == len(positions)
            m = st.s.row_mask(allow)
            try:
                got = part_device(st.s, st.parts["t3"], c.queries, k, flt, mask=m, metric=c.metric)
            finally:
                m.close()
            _same(got, c.topk(st.ref["t3"], flt, k, allow=allow)[:4], f"mask ({label})")
            assert (got[2] == n_found).all(), label
    finally:
        st.s.set_option("partition_blocks", 0)


def test_piece_boundary(pqv):
    """one device call of PARTITION_GRID_Q + 5 queries (32768: the grid's y, restated from csrc/api.cpp) on the smallest rows: 5
    distinct queries and filters, cycled, so the reference is computed for 5 and tiled.  32768 is no multiple of 5: the queries past
    the boundary continue the cycle at its fourth pattern, so each of them has another IN set than the query 32768 places ahead of it
    -- a second piece that read the filter arrays (or IN lims) from the call's start would answer for other keys.  Every output is
    compared whole, and its part past the boundary on its own."""
    piece, n, dim, k = 32768, 300, 8, 3
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
        exp = [tile(x) for x in pr.topk_batch(prows, pkeys, f5[1], f5[2], f5[3], d5, k, "l2", False)[:4]]
        assert exp[2][piece:].max() > 0 and (exp[0][piece:] != EMPTY).any()
        got = part_device(s, part, queries, k, f)
        _same(got, exp, f"{f[0]}: {nq} queries in one device call")
        _same([x[piece:] for x in got], [x[piece:] for x in exp], f"{f[0]}: past the piece boundary")


@pytest.mark.parametrize("nq", [1, 70])
def test_batch_sizes(pqv, oracle, nq):
    st = Setup(pqv, oracle, "1500x30", nq=nq)
    assert st.case.nq == nq
    for col in ("t3", "t64"):
        for flt in st.case.filters(col):
            for k in (10, 100):
                st.check(col, flt, k, blocks=pc.BLOCKS)


@pytest.mark.parametrize("name,layout", [("4096x128", "row"), ("4096x128", "release"), ("1500x30", "row"), ("2048x32-seq", "release")])
def test_layouts(pqv, oracle, name, layout):
    flags = pqv.PQV_LAYOUT_ROW_ORDER if layout == "row" else pqv.PQV_RELEASE_ROW_ORDER
    st = Setup(pqv, oracle, name, flags=flags)
    for col in ("t3", "skew"):
        for flt in st.case.filters(col):
            for k in (10, 300):
                st.check(col, flt, k, what=layout)


@pytest.mark.parametrize("name", ["4096x128", "1500x30"])
def test_removed_rows_are_absent(pqv, oracle, name):
    n = pc.SHAPES[name]["n"]
    removed = np.unique(np.random.default_rng(8).integers(0, n, n // 5))
    st = Setup(pqv, oracle, name, removed=removed)
    for col in st.case.columns:
        assert st.parts[col].rows == len(st.ref[col][0]) < len(st.case.partition(col)[0])
        v, cnt = pr.distinct(st.ref[col][1])
        _same(st.parts[col].keys(), (v, cnt), f"keys() of {col} after a remove")
        for flt in st.case.filters(col):
            got = st.check(col, flt, 100, blocks=(1, 0), what="removed")
            assert not np.isin(got[0][got[0] != EMPTY], removed).any()


@pytest.mark.parametrize("name", pc.LONG_SHAPES)
def test_long_rows_cosine_and_dot(pqv, oracle, name):
    """multi-chunk rows, zero-padded storage ("260"), PQV_COSINE through the cosine layout and PQV_DOT: I32 tenant keys with NULLs,
    and the same keys as an I64 column without"""
    lc = lrc.Case(name, oracle)
    metric = {"l2": lc.metric, "cos": pqv.PQV_COSINE, "dot": pqv.PQV_DOT}[lc.kind]
    d = pr.distances(lc.kind, lc.metric, lc.data, lc.queries)
    corpus = pqv.Corpus.upload(lc.data)
    s = pqv.Searcher(pqv.Index.from_parts(lc.dim, lc.centroids, lc.lists), corpus)
    s1 = one_list(pqv, lc.dim, corpus, np.arange(lc.n))
    lims, vals = kf.sets_to_csr(lrc.QUERY_SETS)
    for values, valid, conv in ((lc.tenant, lc.tenant_valid, lambda v: [int(x) for x in v]),
                                (lrc.wide(lc.tenant), None, lambda v: [int(x) for x in lrc.wide(v)])):
        col = pqv.Column.upload(values, valid)
        part, keys1 = s.key_partition(col), s1.row_keys(col)
        prows, pkeys = pr.build(values, valid, np.arange(lc.n))
        _same(part.keys(), pr.distinct(pkeys), "keys()")
        in_vals = conv(vals) if len(vals) else []
        flts = [("eq", kf.EQ, conv(lrc.QUERY_KEYS), None), ("range", kf.RANGE, conv(lrc.QUERY_RANGES[0]), conv(lrc.QUERY_RANGES[1])),
                ("in", kf.IN, [int(x) for x in lims], in_vals)]
        shared = lc.masks["1/2"]
        m, m1 = s.row_mask(shared), s1.row_mask(shared)
        for flt in flts:
            if flt[1] == kf.IN:     # (wide() is monotonic: the converted slices stay ascending)
                assert all(x < y for i in range(lrc.NQ) for x, y in zip(in_vals[lims[i]:lims[i + 1]], in_vals[lims[i] + 1:lims[i + 1]]))
            for k, sqrt_out in ((10, True), (300, False)):
                for allow, mask, mask1 in ((None, None, None), (shared, m, m1)):
                    exp = pr.topk_batch(prows, pkeys, flt[1], flt[2], flt[3], d, k, lc.kind, sqrt_out, allow)
                    for b in pc.BLOCKS:
                        s.set_option("partition_blocks", b)
                        got = part_device(s, part, lc.queries, k, flt, mask=mask, metric=metric, sqrt_out=sqrt_out)
                        _same(got, exp[:4], f"{name} {flt[0]} k={k} blocks={b}")
                    s.set_option("partition_blocks", 0)
                    host = s.topk_partition(lc.queries, k, part, mask=mask, metric=metric, sqrt_out=sqrt_out, **_host_filter(flt))
                    _same(host, got, f"{name} {flt[0]} k={k} host form")
                    if lc.kind != "dot":
                        twin = s1_device(s1, lc.queries, k, keys=keys1, flt=flt, mask=mask1, metric=metric, sqrt_out=sqrt_out)
                        _same(got[:3], twin, f"{name} {flt[0]} k={k} vs the filtered call on S1")
                    elif k == 10:       # the keyed calls refuse PQV_DOT: the masked call on S1, per query under M_q
                        for q in range(lrc.NQ):
                            mq = s1.row_mask(kf.allowed_for(values, valid, flt[1], flt[2], flt[3], q, allow))
                            twin = s1_device(s1, lc.queries[q:q + 1], k, mask=mq, metric=metric, sqrt_out=sqrt_out)
                            mq.close()
                            _same([x[q:q + 1] for x in got[:3]], twin, f"{name} {flt[0]} query {q} vs the masked call on S1")
        m.close()
        m1.close()


def test_ties_follow_distance_then_position(pqv):
    data, queries, keys = pc.tie_case()
    corpus = pqv.Corpus.upload(data)
    n, dim = data.shape
    lists = [np.arange(i, n, 3, dtype=np.uint32) for i in range(3)]
    s = pqv.Searcher(pqv.Index.from_parts(dim, np.zeros((3, dim), np.float32), lists), corpus)
    part = s.key_partition(pqv.Column.upload(keys))
    prows, pkeys = pr.build(keys, None, np.arange(n))
    d = pr.distances("l2", pr.REF4, data, queries)
    assert any(len(np.unique(row)) < len(row) // 4 for row in d), "the case is about equal distances"
    lims, vals = kf.sets_to_csr([[0, 3], [1], [0, 1, 2, 3], [2, 9], []])
    for flt in (("eq", kf.EQ, [0, 1, 2, 3, 7], None), ("range", kf.RANGE, [0, 1, 0, 3, 2], [1, 3, 3, 3, 1]),
                ("in", kf.IN, [int(x) for x in lims], [int(x) for x in vals])):
        for k in (1, 10, 100):
            for b in pc.BLOCKS:
                s.set_option("partition_blocks", b)
                exp = pr.topk_batch(prows, pkeys, flt[1], flt[2], flt[3], d, k, "l2", True)
                _same(part_device(s, part, queries, k, flt, sqrt_out=True), exp[:4], f"ties {flt[0]} k={k} blocks={b}")
                _same(s.topk_partition(queries, k, part, **_host_filter(flt)), exp[:4], f"ties {flt[0]} k={k} host")


def test_device_filter_arrays_written_on_the_call_stream(shape):
    """the descriptor's device arrays are read inside the enqueued work: written on the same stream just before the call, with no
    synchronisation in between"""
    import torch
    st, c = shape, shape.case
    stream = torch.cuda.Stream()
    for flt in c.filters("t64"):
        exp = c.topk(st.ref["t64"], flt, 10)
        a_host = torch.tensor([int(x) for x in flt[2]], dtype=torch.int64).pin_memory()
        b_host = torch.tensor([int(x) for x in (flt[3] or [0])] or [0], dtype=torch.int64).pin_memory()
        q_host = torch.from_numpy(c.queries).pin_memory()
        out = _outputs(c.nq, 10)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            a_t = torch.zeros_like(a_host, device=_dev())
            b_t = torch.zeros_like(b_host, device=_dev())
            q_t = torch.zeros_like(q_host, device=_dev())
            a_t.copy_(a_host, non_blocking=True)
            b_t.copy_(b_host, non_blocking=True)
            q_t.copy_(q_host, non_blocking=True)
            kw = {kf.EQ: dict(query_keys=a_t.data_ptr()), kf.RANGE: dict(query_key_ranges=(a_t.data_ptr(), b_t.data_ptr())),
                  kf.IN: dict(query_key_sets=(a_t.data_ptr(), b_t.data_ptr()))}[flt[1]]
            st.s.topk_partition_device(q_t.data_ptr(), c.nq, 10, st.parts["t64"], out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                       out[3].data_ptr(), metric=c.metric, sqrt_out=False, stream=stream.cuda_stream, **kw)
        stream.synchronize()
        _same(_results(*out), exp[:4], f"{flt[0]} on a caller's stream")


def test_lifetime_refusals_and_limits(pqv, oracle):
    c = pc.Case("1500x30")
    built = oracle.build_index(c.data, n_clusters=c.kc, max_iters=5, workers=1)
    lists = [np.asarray(l, np.uint32) for l in built.lists()]
    corpus = pqv.Corpus.upload(c.data)
    index = pqv.Index.from_parts(c.dim, built.centroids, lists)
    col = pqv.Column.upload(*c.columns["t64"])
    flt = c.filters("t64")[0]
    exp = c.topk(c.partition("t64"), flt, 10)
    # the partition freed before its searcher, and after it
    s = pqv.Searcher(index, corpus)
    p1, p2 = s.key_partition(col), s.key_partition(col)
    col.close()                                 # (the column is not kept)
    _same(part_device(s, p2, c.queries, 10, flt), exp[:4])
    p1.close()
    _same(part_device(s, p2, c.queries, 10, flt), exp[:4])
    other = pqv.Searcher(index, corpus)
    with pytest.raises(pqv.PqvError, match="key partition belongs to another searcher"):
        other.topk_partition(c.queries, 10, p2, query_keys=flt[2])
    om = other.row_mask(np.ones(c.n, bool))
    with pytest.raises(pqv.PqvError, match="row mask belongs to another searcher"):
        s.topk_partition(c.queries, 10, p2, query_keys=flt[2], mask=om)
    om.close()
    other.close()
    # k beyond the kernels' lists: both forms refuse, there is no host fallback
    for call in (lambda k: s.topk_partition(c.queries, k, p2, query_keys=flt[2]), lambda k: part_device(s, p2, c.queries, k, flt)):
        with pytest.raises(pqv.PqvError, match="pqv_topk_partition takes k <= 1024") as e:
            call(1025)
        assert e.value.code == pqv._ffi.PQV_ERR_UNSUPPORTED
        with pytest.raises(pqv.PqvError, match="k must be > 0"):
            call(0)
    with pytest.raises(pqv.PqvError, match="Query dimension mismatch: expected 30, got 29"):
        s.topk_partition(c.queries[:, :29], 10, p2, query_keys=flt[2])
    with pytest.raises(pqv.PqvError, match="unknown metric"):
        s.topk_partition(c.queries, 10, p2, query_keys=flt[2], metric=9)
    assert s.topk_partition(c.queries[:0], 10, p2, query_keys=[])[0].shape == (0, 10)
    with pytest.raises(pqv.PqvError, match="key column must be PQV_COL_I32 or PQV_COL_I64"):
        s.key_partition(pqv.Column.upload(np.zeros(c.n, np.float32)))
    with pytest.raises(pqv.PqvError, match="column has 7 rows, the corpus has 1500"):
        s.key_partition(pqv.Column.upload(np.zeros(7, np.int32)))
    s.close()
    assert p2.rows == len(c.partition("t64")[0]) and len(p2.keys()[0]) == p2.n_keys       # (still readable behind its searcher)
    p2.close()
    # table searchers are refused
    t = pqv.TableSearcher([index], corpus, [0])
    with pytest.raises(pqv.PqvError, match="pqv_key_partition_create does not take table searchers") as e:
        t.key_partition(pqv.Column.upload(c.columns["t3"][0]))
    assert e.value.code == pqv._ffi.PQV_ERR_UNSUPPORTED
    t.close()
    # a column of NULLs only: an empty partition answers nothing
    s = pqv.Searcher(index, corpus)
    empty = s.key_partition(pqv.Column.upload(np.zeros(c.n, np.int64), np.zeros(c.n, np.uint8)))
    assert empty.rows == 0 and empty.n_keys == 0 and len(empty.keys()[0]) == 0
    got = part_device(s, empty, c.queries, 10, ("eq", kf.EQ, [0] * c.nq, None))
    assert (got[2] == 0).all() and (got[3] == 0).all() and (got[0] == EMPTY).all() and np.isposinf(got[1]).all()
    empty.close()
    s.close()


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
def test_host_sub_batches(pqv, oracle, masked):
    """One host call of more queries than one sub-batch of pqv_topk_partition holds (1500 x 30, partition_blocks 16, k = 256: the
    per-query scratch against the 1 GiB bound, restated from csrc/api.cpp), for EQ, RANGE and IN filters that cycle over five
    patterns (sets of 1, 2, 0, 3 and 5 values): the second sub-batch is right only if it got its own slice of the filter arrays,
    IN lims rebased, and wrote at its offsets.  Compared with the restatement for the first 64 queries, the 64 on each side of
    q0 = batch and the last 64, and for every query with the concatenation of calls of at most 1000 queries."""
    name, k, blocks = "1500x30", 256, 16
    c = pc.SHAPES[name]
    sdim = c["dim"]                          # (30 dims: stored as they are)
    per_query = blocks * 4 * k * 12 + sdim * 8 + 12 * k + 8 * 1024          # (1024: PQV_KEY_SET_MAX)
    batch = min(32768, (1 << 30) // per_query)
    assert 1000 < batch < 8000
    nq = batch + batch // 2                  # (the second sub-batch starts in the middle of the call)
    st = Setup(pqv, oracle, name, nq=1)
    data = st.case.data
    q = np.random.default_rng(91).random((nq, c["dim"]), dtype=np.float32)
    sel = np.concatenate([np.arange(0, 64), np.arange(batch - 64, batch + 64), np.arange(nq - 64, nq)])
    d_sel = pr.distances("l2", c["metric"], data, q[sel])
    allow = np.random.default_rng(92).random(c["n"]) < 0.5 if masked else None
    mask = st.s.row_mask(allow) if masked else None
    col = "t3"
    prows, pkeys = st.ref[col]
    st.s.set_option("partition_blocks", blocks)
    try:
        for flt in pc.filters(col, nq, 93):
            _, kind, a, b = flt

            def sub(lo, hi):                 # the filter of the queries [lo, hi)
                if kind == kf.IN:
                    return (flt[0], kind, [x - a[lo] for x in a[lo:hi + 1]], b[a[lo]:a[hi]])
                return (flt[0], kind, a[lo:hi], b[lo:hi] if b is not None else None)

            def call(lo, hi):
                return st.s.topk_partition(q[lo:hi], k, st.parts[col], mask=mask, metric=c["metric"], sqrt_out=False, **_host_filter(sub(lo, hi)))

            got = call(0, nq)
            small = [call(lo, min(lo + 1000, nq)) for lo in range(0, nq, 1000)]
            _same(got, [np.concatenate([p[j] for p in small]) for j in range(4)], f"{flt[0]}: one call vs smaller calls")
            for j, i in enumerate(sel):
                exp = pr.topk(prows, pkeys, kind, a, b, int(i), d_sel[j], k, "l2", False, allow)
                _same([x[i:i + 1] for x in got], [exp[0][None], exp[1][None], np.array([exp[2]], np.uint32), np.array([exp[3]], np.uint64)],
                      f"{flt[0]}: query {i} vs the restatement")
            assert (got[2][batch:] > 0).any()
            if kind == kf.RANGE:             # (the full range: more than k rows also under the mask)
                assert (got[2][batch:] == k).any()
    finally:
        st.s.set_option("partition_blocks", 0)
        if mask is not None:
            mask.close()
