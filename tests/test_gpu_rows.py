"""Candidate lists on the GPU (pqv_topk_rows, pqv_topk_rows_device, pqv_score_rows, pqv_score_rows_device).

Every call is compared, bit for bit, against the numpy restatement (tests/rows_ref.py) over the inputs of the key partition tests
(tests/partition_cases.py: no two rows of a case equally far from a query) and the lists of tests/rows_cases.py, and against the
calls the contract names as twins: pqv_topk_masked_device on S1 -- a searcher over Index.from_parts(dim, one centroid, [all
indexed rows ascending]) on the same corpus, nprobe = 1 -- per query under the mask M_q = the list, and pqv_topk_partition where a
list is one key's rows.  Lists with duplicates have equal distances by construction: there both sides order by (distance key,
position), which is what the contract states.  There are no tolerances."""
import numpy as np
import pytest

import long_rows_cases as lrc
import partition_cases as pc
import partition_ref as pr
import rows_cases as rc
import rows_ref as rr

pytestmark = pytest.mark.gpu

EMPTY = 0xFFFFFFFF


def _same(got, exp, what=""):
    for i, (x, y) in enumerate(zip(got, exp)):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and (x.view(np.uint8) == y.view(np.uint8)).all(), f"{what}: output {i} differs"


def _dev():
    import torch
    return torch.device("cuda", 0)


def _outputs(nq, k):
    import torch
    dev = _dev()
    return (torch.full((nq, k), 7, dtype=torch.int32, device=dev), torch.full((nq, k), -1.0, dtype=torch.float32, device=dev),
            torch.full((nq,), 7, dtype=torch.int32, device=dev), torch.full((nq,), 7, dtype=torch.int64, device=dev))


def _results(r_t, d_t, nf_t, nc_t):
    return (r_t.cpu().numpy().view(np.uint32), d_t.cpu().numpy(), nf_t.cpu().numpy().astype(np.uint32), nc_t.cpu().numpy().astype(np.uint64))


def _device_lists(lims, rows):
    """(lims tensor, rows tensor): u64 / u32 arrays as int64 / int32 bits (lims are below 2^63); one id of padding keeps the rows'
    pointer non-NULL for a call whose slices are all empty"""
    import torch
    return (torch.from_numpy(np.ascontiguousarray(lims, np.uint64).view(np.int64).copy()).to(_dev()),
            torch.from_numpy(np.concatenate([np.asarray(rows, np.uint32), np.zeros(1, np.uint32)]).view(np.int32).copy()).to(_dev()))


def rows_device(s, lists, q, k, mask=None, metric=0, sqrt_out=False, base=0):
    """topk_rows_device -> (rows, dist, n_found, n_candidates); lists: per-query arrays, or a (lims, rows) tuple"""
    import torch
    lims, rows = lists if isinstance(lists, tuple) else rr.csr(lists, base)
    q_t = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(_dev())
    l_t, r_t = _device_lists(lims, rows)
    out = _outputs(len(q), k)
    torch.cuda.synchronize()
    s.topk_rows_device(q_t.data_ptr(), len(q), k, l_t.data_ptr(), r_t.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                       out[3].data_ptr(), mask=mask, metric=metric, sqrt_out=sqrt_out)
    torch.cuda.synchronize()
    return _results(*out)


def score_device(s, lists, q, mask=None, metric=0, sqrt_out=False, base=0):
    """score_rows_device -> dist f32 [total]; the output starts as -1 everywhere: every slot must be written"""
    import torch
    lims, rows = rr.csr(lists, base)
    total = int(lims[-1] - lims[0])
    q_t = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(_dev())
    l_t, r_t = _device_lists(lims, rows)
    out = torch.full((total + 3,), -1.0, dtype=torch.float32, device=_dev())
    torch.cuda.synchronize()
    s.score_rows_device(q_t.data_ptr(), len(q), l_t.data_ptr(), r_t.data_ptr(), out.data_ptr(), mask=mask, metric=metric, sqrt_out=sqrt_out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[total:] == -1.0).all(), "the score form wrote past its output"
    return got[:total]


def s1_masked(s1, q, k, mask, metric=0, sqrt_out=False):
    """topk_device on S1 with nprobe = 1 under `mask` -> (rows, dist, n_found)"""
    import torch
    q_t = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(_dev())
    out = _outputs(len(q), k)
    torch.cuda.synchronize()
    s1.topk_device(q_t.data_ptr(), len(q), k, 1, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), metric=metric,
                   sqrt_out=sqrt_out, mask=mask)
    torch.cuda.synchronize()
    return _results(*out)[:3]


def one_list(pqv, dim, corpus, indexed, flags=0):
    """S1 of the contract: one list = all indexed rows ascending, any centroid"""
    rows = np.sort(np.asarray(indexed)).astype(np.uint32)
    return pqv.Searcher(pqv.Index.from_parts(dim, np.zeros((1, dim), np.float32), [rows]), corpus, flags)


class Setup:
    """A case on the device: the corpus, an index over the case's lists (less `removed`) and its searcher; S1 on demand.  d: the
    distance matrix [nq, n] before the output transform, kind: "l2" / "cos" / "dot"."""

    def __init__(self, pqv, data, queries, centroids, lists, metric, kind, d, flags=0, removed=None):
        self.pqv, self.data, self.queries, self.metric, self.kind, self.d = pqv, data, queries, metric, kind, d
        self.n, self.dim, self.nq = len(data), data.shape[1], len(queries)
        self.corpus = pqv.Corpus.upload(data)
        index = pqv.Index.from_parts(self.dim, centroids, [np.asarray(l, np.uint32) for l in lists])
        self.indexed_rows = np.arange(self.n)
        if removed is not None:
            index = index.remove(rows=removed)
            self.indexed_rows = np.setdiff1d(self.indexed_rows, removed)
        self.indexed = np.zeros(self.n, bool)
        self.indexed[self.indexed_rows] = True
        self.index, self.flags = index, flags
        self._s1 = None
        self.s = pqv.Searcher(index, self.corpus, flags)

    @property
    def s1(self):
        if self._s1 is None:
            corpus = self.corpus
            if self.flags & self.pqv.PQV_RELEASE_ROW_ORDER:      # (the searcher took the corpus' rows with it: S1 reads a copy of its own)
                corpus = self._s1_corpus = self.pqv.Corpus.upload(self.data)
            self._s1 = one_list(self.pqv, self.dim, corpus, self.indexed_rows)
        return self._s1

    def check(self, lists, k, allow=None, mask=None, sqrt_out=False, base=0, blocks=(0,), host=True, what=""):
        """the device form under every `blocks` == the restatement == the host form"""
        exp = rr.topk_batch(lists, self.indexed, self.d, k, self.kind, sqrt_out, allow)
        for b in blocks:
            self.s.set_option("partition_blocks", b)
            got = rows_device(self.s, lists, self.queries, k, mask=mask, metric=self.metric, sqrt_out=sqrt_out, base=base)
            _same(got, exp[:4], f"{what} k={k} blocks={b} device form vs the restatement")
        self.s.set_option("partition_blocks", 0)
        if host:
            h = self.s.topk_rows(self.queries, k, rr.csr(lists, base) if base else lists, mask=mask, metric=self.metric, sqrt_out=sqrt_out)
            _same(h, got, f"{what} k={k} host form vs device form")
        return got

    def check_scores(self, lists, allow=None, mask=None, sqrt_out=False, base=0, blocks=(0,), what=""):
        """both score forms under every `blocks` == the restatement"""
        lims, exp = rr.scores_batch(lists, self.indexed, self.d, self.kind, sqrt_out, allow)
        for b in blocks:
            self.s.set_option("partition_blocks", b)
            got = score_device(self.s, lists, self.queries, mask=mask, metric=self.metric, sqrt_out=sqrt_out, base=base)
            _same([got], [exp], f"{what} blocks={b} score device form vs the restatement")
        self.s.set_option("partition_blocks", 0)
        hl, hd = self.s.score_rows(self.queries, rr.csr(lists, base) if base else lists, mask=mask, metric=self.metric, sqrt_out=sqrt_out)
        _same([hl, hd], [lims, exp], f"{what} score host form vs the restatement")
        return got


def shape_setup(pqv, oracle, name, nq=5, flags=0, removed=None):
    c = pc.Case(name, nq)
    built = oracle.build_index(c.data, n_clusters=c.kc, max_iters=5, workers=1)
    return Setup(pqv, c.data, c.queries, built.centroids, built.lists(), c.metric, "l2", c.d, flags, removed)


def long_setup(pqv, oracle, name):
    lc = lrc.Case(name, oracle)
    metric = {"l2": lc.metric, "cos": pqv.PQV_COSINE, "dot": pqv.PQV_DOT}[lc.kind]
    return Setup(pqv, lc.data, lc.queries, lc.centroids, lc.lists, metric, lc.kind, pr.distances(lc.kind, lc.metric, lc.data, lc.queries))


@pytest.fixture(scope="module", params=list(pc.SHAPES))
def shape(request, pqv, oracle):
    return shape_setup(pqv, oracle, request.param)


@pytest.fixture(scope="module", params=pc.LONG_SHAPES)
def long_shape(request, pqv, oracle):
    return long_setup(pqv, oracle, request.param)


def _list_sets(n):
    """(label, lists, base): unsorted unique lists of every slice length, and messy ones (duplicates, ids that are no rows) behind a
    lims that starts at 7"""
    return (("unique A", rc.unique_lists(n, rc.LENS_A, 21), 0), ("unique B", rc.unique_lists(n, rc.LENS_B, 22), 0),
            ("messy A", rc.messy_lists(n, rc.LENS_A, 23), 7), ("messy B", rc.messy_lists(n, rc.LENS_B, 24), 0))


def _against_the_restatement(st):
    for label, lists, base in _list_sets(st.n):
        for k in rc.KS:
            got = st.check(lists, k, base=base, blocks=(1, 2, 0) if k in (10, 65) else (0,), sqrt_out=k == 64, what=label)
            rows, dist, nf, nc = got
            assert (nc == [len(l) for l in lists]).all() and (nf <= np.minimum(k, nc)).all()
            for q in range(st.nq):
                assert (rows[q, nf[q]:] == EMPTY).all() and np.isposinf(dist[q, nf[q]:]).all()
        for sqrt_out in (False, True):
            st.check_scores(lists, base=base, sqrt_out=sqrt_out, blocks=(1, 2, 0), what=label)
    assert st.check(rc.unique_lists(st.n, rc.LENS_A, 21), 1024)[2].tolist() == list(rc.LENS_A), "k above the slice length: every candidate"


def test_against_the_restatement(shape):
    """host and device top-k and both score forms; slices of 0, 1, 63, 64, 65, 255, 256, 257 and about 1000 candidates; k in {1, 10,
    64, 65, 1024}; partition_blocks 1, 2 and by rule; unsorted lists, duplicates, ids that are no rows, a lims that starts at 7"""
    _against_the_restatement(shape)


def test_long_rows_cosine_and_dot_against_the_restatement(long_shape):
    """multi-chunk rows, zero-padded storage ("260"), PQV_COSINE through the cosine layout and PQV_DOT"""
    _against_the_restatement(long_shape)


@pytest.mark.parametrize("name", ["4096x128", "1500x30"])
def test_one_query(pqv, oracle, name):
    st = shape_setup(pqv, oracle, name, nq=1)
    for lens in ((1000,), (65,), (0,)):
        for lists in (rc.unique_lists(st.n, lens, 31), rc.messy_lists(st.n, lens, 32)):
            for k in rc.KS:
                st.check(lists, k, blocks=(1, 2, 0))
            st.check_scores(lists, blocks=(1, 2, 0))


def _against_masked_search_on_s1(st, ks=(1, 10, 65)):
    lists = rc.unique_lists(st.n, rc.LENS_B, 41, ascending=True)
    for k in ks:
        got = rows_device(st.s, lists, st.queries, k, metric=st.metric, sqrt_out=True)
        for q, l in enumerate(lists):
            m_q = np.zeros(st.n, bool)
            m_q[l] = True
            mq = st.s1.row_mask(m_q)
            try:
                twin = s1_masked(st.s1, st.queries[q:q + 1], k, mq, metric=st.metric, sqrt_out=True)
            finally:
                mq.close()
            _same([x[q:q + 1] for x in got[:3]], twin, f"k={k} query {q} vs the masked call on S1")


def test_ascending_lists_equal_masked_search_on_s1(shape):
    _against_masked_search_on_s1(shape)


def test_ascending_lists_equal_masked_search_on_s1_long_rows(long_shape):
    """... PQV_COSINE and PQV_DOT among them: all four metrics"""
    _against_masked_search_on_s1(long_shape)


def test_a_keys_rows_equal_the_partition_call(shape, pqv):
    """each list = one key's rows ascending: the partition call with PQV_KEY_EQ on the same searcher, bit for bit"""
    st = shape
    values = pc.columns(st.n, 5000 + st.dim + 17)["t3"][0]
    col = pqv.Column.upload(values)
    part = st.s.key_partition(col)
    try:
        keys = [-5, 0, 7, 3, 7][:st.nq]              # (3 is no key of the column: an empty list)
        lists = [np.sort(st.indexed_rows[values[st.indexed_rows] == key]).astype(np.uint32) for key in keys]
        assert min(len(l) for l in lists) == 0 and max(len(l) for l in lists) > 256
        for k in (1, 10, 300):
            for sqrt_out in (False, True):
                twin = st.s.topk_partition(st.queries, k, part, query_keys=keys, metric=st.metric, sqrt_out=sqrt_out)
                _same(rows_device(st.s, lists, st.queries, k, metric=st.metric, sqrt_out=sqrt_out), twin, f"k={k} vs pqv_topk_partition")
                _same(st.s.topk_rows(st.queries, k, lists, metric=st.metric, sqrt_out=sqrt_out), twin, f"k={k} host form vs pqv_topk_partition")
    finally:
        part.close()
        col.close()


def test_ties_follow_distance_then_position_as_the_partition_call(pqv):
    data, queries, keys = pc.tie_case()
    corpus = pqv.Corpus.upload(data)
    n, dim = data.shape
    lists3 = [np.arange(i, n, 3, dtype=np.uint32) for i in range(3)]
    s = pqv.Searcher(pqv.Index.from_parts(dim, np.zeros((3, dim), np.float32), lists3), corpus)
    part = s.key_partition(pqv.Column.upload(keys))
    d = pr.distances("l2", pr.REF4, data, queries)
    assert any(len(np.unique(row)) < len(row) // 4 for row in d), "the case is about equal distances"
    qkeys = [0, 1, 2, 3, 7]
    lists = [np.nonzero(keys == key)[0].astype(np.uint32) for key in qkeys]
    indexed = np.ones(n, bool)
    for k in (1, 10, 100):
        for b in (1, 2, 0):
            s.set_option("partition_blocks", b)
            twin = s.topk_partition(queries, k, part, query_keys=qkeys)
            exp = rr.topk_batch(lists, indexed, d, k, "l2", True)
            _same(twin, exp[:4], f"ties k={k}: the two restatements")
            _same(rows_device(s, lists, queries, k, sqrt_out=True), twin, f"ties k={k} blocks={b} vs pqv_topk_partition")
            _same(s.topk_rows(queries, k, lists), twin, f"ties k={k} blocks={b} host form")
    # an unsorted list with duplicates over the tied rows: (distance, position) alone decides
    messy = rc.messy_lists(n, rc.LENS_B, 51)
    for k in (10, 300):
        _same(rows_device(s, messy, queries, k), rr.topk_batch(messy, indexed, d, k, "l2", False)[:4], f"ties, messy lists, k={k}")


def _scores_against_topk(st):
    for label, lists, base in _list_sets(st.n):
        for sqrt_out in (False, True):
            sc = score_device(st.s, lists, st.queries, metric=st.metric, sqrt_out=sqrt_out, base=base)
            rows, dist, nf, _ = rows_device(st.s, lists, st.queries, 1024, metric=st.metric, sqrt_out=sqrt_out, base=base)
            lims = np.concatenate([[0], np.cumsum([len(l) for l in lists])])
            for q, l in enumerate(lists):
                mine = sc[lims[q]:lims[q + 1]]
                assert nf[q] == (~np.isposinf(mine)).sum(), (label, q)
                # per candidate: the distance the top-k call reports for its row (a row listed twice has one distance)
                of_row = dict(zip(rows[q, :nf[q]].tolist(), dist[q, :nf[q]].view(np.uint32).tolist()))
                for i, r in enumerate(l.tolist()):
                    if not np.isposinf(mine[i]):
                        assert of_row[r] == int(mine[i:i + 1].view(np.uint32)[0]), (label, q, i)
                if not sqrt_out:
                    er, ed, en = rr.topk_from_scores(l, mine, 1024, st.kind)
                    assert nf[q] == en
                    _same([rows[q], dist[q]], [er, ed], f"{label} query {q}: top-k vs the stable sort of the scores")


def test_scores_are_the_topk_distances(shape):
    _scores_against_topk(shape)


def test_scores_are_the_topk_distances_long_rows(long_shape):
    _scores_against_topk(long_shape)


@pytest.mark.parametrize("name", ["4096x128", "1500x30"])
def test_unindexed_rows_are_skipped(pqv, oracle, name):
    """rows at or above the row bound, 0xFFFFFFFF and removed rows: counted in n_candidates, not in embeddings_fetched, +inf scores"""
    n = pc.SHAPES[name]["n"]
    removed = np.unique(np.random.default_rng(8).integers(0, n, n // 5))
    st = shape_setup(pqv, oracle, name, removed=removed)
    assert st.index.row_bound <= n
    lists = rc.messy_lists(n, rc.LENS_B, 61, bound=st.index.row_bound)
    lists[0] = np.concatenate([lists[0], removed[:40].astype(np.uint32)])
    flat = np.concatenate(lists)
    assert np.isin(flat, removed).any() and (flat == EMPTY).any() and (flat >= n).any()
    for k in (10, 300, 1024):
        before = st.s.counters()
        got = st.check(lists, k, blocks=(1, 0), host=False, what="removed")
        after = st.s.counters()
        exp = rr.topk_batch(lists, st.indexed, st.d, k)
        assert not np.isin(got[0][got[0] != EMPTY], removed).any() and (got[0][got[0] != EMPTY] < n).all()
        assert (got[3] == [len(l) for l in lists]).all()
        assert after["queries"] - before["queries"] == 2 * st.nq
        assert after["candidate_rows"] - before["candidate_rows"] == 2 * len(flat)
        assert after["embeddings_fetched"] - before["embeddings_fetched"] == 2 * exp[4] < 2 * len(flat)
    sc = st.check_scores(lists, blocks=(1, 0), what="removed")
    assert np.isposinf(sc[np.isin(flat, removed) | (flat >= n)]).all() and not np.isposinf(sc).all()
    only_gone = [removed[:70].astype(np.uint32)] + [np.array([EMPTY, n], np.uint32)] * (st.nq - 1)
    got = st.check(only_gone, 10, what="lists of unindexed rows only")
    assert (got[2] == 0).all() and (got[3] == [70] + [2] * (st.nq - 1)).all()


def test_appended_and_compacted_indexes(pqv, oracle):
    """the states of tests/mutated_cases.py (exact30): rows that joined by an append, rows two removes took out -- an emptied list
    among them --, and the renumbered rows of a compacted index"""
    from test_gpu_mutated_search import Zoo
    zoo = Zoo(pqv, oracle, "exact30", searchers=False)
    c = zoo.case
    # (an appended index takes a corpus of exactly its rows: the zoo's has grown on, so the state is made again on one that has not)
    corpus = pqv.Corpus.create(c.n1, c.dim)
    try:
        corpus.append(c.X[:c.n0])
        built = pqv.IndexBuilder(corpus).n_clusters(c.kc).max_iters(5).workers(1).build()
        corpus.append(c.X[c.n0:c.n1])
        appended = built.append(corpus)
        assert appended.to_bytes() == zoo.index["appended"].to_bytes()
        _mutated_state(pqv, "appended", appended, corpus, c.models["appended"], c.Q[:5])
        _mutated_state(pqv, "chained", zoo.index["chained"], zoo.corpus, c.models["chained"], c.Q[:5])
        _mutated_state(pqv, "compacted", zoo.index["compacted"], zoo.dense, c.models["compacted"], c.Q[:5])
        appended.close()
        built.close()
    finally:
        corpus.close()
        zoo.close()


def _mutated_state(pqv, state, index, corpus, m, queries):
    """one state: a searcher over it, candidate lists with ids past its bound and rows it does not index"""
    s = pqv.Searcher(index, corpus)
    n = corpus.rows
    indexed, X = np.zeros(n, bool), np.zeros((n, m.dim), np.float32)
    have = min(n, m.n)
    indexed[:have], X[:have] = m.in_lists()[:have], m.X[:have]
    assert indexed.sum() == sum(len(l) for l in m.lists) <= n and m.bound <= n
    d = pr.distances("l2", pr.REF4, X, queries)
    lists = rc.messy_lists(n, rc.LENS_B, 71, bound=m.bound)
    lists[1] = np.concatenate([lists[1], np.nonzero(~indexed)[0][:50].astype(np.uint32)])
    for k in (10, 300):
        exp = rr.topk_batch(lists, indexed, d, k, "l2", True)
        _same(rows_device(s, lists, queries, k, sqrt_out=True), exp[:4], f"{state} k={k}")
        _same(s.topk_rows(queries, k, lists), exp[:4], f"{state} k={k} host form")
    _same([score_device(s, lists, queries)], [rr.scores_batch(lists, indexed, d)[1]], f"{state} scores")
    s.close()


@pytest.mark.parametrize("layout", ["ivf", "row", "release"])
def test_shared_mask_and_layouts(pqv, oracle, layout):
    """a mask allows about half the rows, and one allows none: considered candidates keep their unmasked positions, n_candidates is
    taken before the mask; on one searcher a cosine call before and after the L2 calls"""
    flags = {"ivf": 0, "row": pqv.PQV_LAYOUT_ROW_ORDER, "release": pqv.PQV_RELEASE_ROW_ORDER}[layout]
    st = shape_setup(pqv, oracle, "4096x128", flags=flags)
    cos = Setup.__new__(Setup)
    cos.__dict__.update(st.__dict__)
    cos.metric, cos.kind, cos.d = pqv.PQV_COSINE, "cos", pr.distances("cos", pr.REF4, st.data, st.queries)
    lists = rc.messy_lists(st.n, rc.LENS_B, 81)
    cos.check(lists, 10, what=f"{layout} cosine first")
    for allow in (np.random.default_rng(3).random(st.n) < 0.5, np.zeros(st.n, bool)):
        m = st.s.row_mask(allow)
        try:
            for k in (10, 300):
                got = st.check(lists, k, allow=allow, mask=m, blocks=(1, 2, 0), what=f"{layout} masked")
                assert (got[3] == [len(l) for l in lists]).all()
                if not allow.any():
                    assert (got[2] == 0).all()
            st.check_scores(lists, allow=allow, mask=m, sqrt_out=True, what=f"{layout} masked")
            cos.check(lists, 10, allow=allow, mask=m, what=f"{layout} cosine masked")
            cos.check_scores(lists, allow=allow, mask=m, what=f"{layout} cosine masked")
        finally:
            m.close()
    st.check(lists, 65, what=f"{layout} L2 behind cosine")
    cos.check(lists, 65, what=f"{layout} cosine behind L2")
    _against_masked_search_on_s1(st, ks=(10,))


def test_counters_and_the_map_build_disturbs_nothing(pqv, oracle):
    st = shape_setup(pqv, oracle, "2048x256")
    first = st.s.topk(st.queries, 10, 2)                      # (before the searcher has a row map)
    lists = rc.messy_lists(st.n, rc.LENS_A, 91)
    flat = np.concatenate(lists)
    m = st.s.row_mask(np.random.default_rng(5).random(st.n) < 0.25)
    try:
        for mask, allow in ((None, None), (m, m.to_bytes().astype(bool))):
            exp = rr.topk_batch(lists, st.indexed, st.d, 10, "l2", False, allow)
            before = st.s.counters()
            a = rows_device(st.s, lists, st.queries, 10, mask=mask)
            mid = st.s.counters()
            b = rows_device(st.s, lists, st.queries, 10, mask=mask)
            _same(a, b, "the same call twice")
            _same(a, exp[:4], "vs the restatement")
            _same(st.s.topk_rows(st.queries, 10, lists, mask=mask, sqrt_out=False), a, "host form")
            after = st.s.counters()
            score_device(st.s, lists, st.queries, mask=mask)
            st.s.score_rows(st.queries, lists, mask=mask)
            scored = st.s.counters()
            for lo, hi, calls in ((before, mid, 1), (mid, after, 2), (after, scored, 2)):
                assert hi["queries"] - lo["queries"] == calls * st.nq
                assert hi["candidate_rows"] - lo["candidate_rows"] == calls * len(flat)
                assert hi["embeddings_fetched"] - lo["embeddings_fetched"] == calls * exp[4]
                assert hi["screened_pairs"] == lo["screened_pairs"] and hi["screen_survivors"] == lo["screen_survivors"]
                assert hi["exact_replays"] == lo["exact_replays"]
    finally:
        m.close()
    _same(st.s.topk(st.queries, 10, 2), first, "an L2 top-k before and after the first candidate-list call")


def test_device_lists_written_on_the_call_stream(shape):
    """d_lims and d_cand_rows are read inside the enqueued work: written on the same stream just before the call, with no
    synchronisation in between"""
    import torch
    st = shape
    lists = rc.messy_lists(st.n, rc.LENS_B, 95)
    rows_device(st.s, lists[:1], st.queries[:1], 1, metric=st.metric)         # (the searcher's first call builds its map and waits)
    lims, rows = rr.csr(lists)
    exp = rr.topk_batch(lists, st.indexed, st.d, 10)
    exp_sc = rr.scores_batch(lists, st.indexed, st.d)[1]
    stream = torch.cuda.Stream()
    l_host = torch.from_numpy(lims.view(np.int64).copy()).pin_memory()
    r_host = torch.from_numpy(rows.view(np.int32).copy()).pin_memory()
    q_host = torch.from_numpy(st.queries).pin_memory()
    out = _outputs(st.nq, 10)
    sc = torch.full((len(rows),), -1.0, dtype=torch.float32, device=_dev())
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        l_t = torch.zeros_like(l_host, device=_dev())
        r_t = torch.zeros_like(r_host, device=_dev())
        q_t = torch.zeros_like(q_host, device=_dev())
        l_t.copy_(l_host, non_blocking=True)
        r_t.copy_(r_host, non_blocking=True)
        q_t.copy_(q_host, non_blocking=True)
        st.s.topk_rows_device(q_t.data_ptr(), st.nq, 10, l_t.data_ptr(), r_t.data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                              out[2].data_ptr(), out[3].data_ptr(), metric=st.metric, sqrt_out=False, stream=stream.cuda_stream)
        st.s.score_rows_device(q_t.data_ptr(), st.nq, l_t.data_ptr(), r_t.data_ptr(), sc.data_ptr(), metric=st.metric, sqrt_out=False,
                               stream=stream.cuda_stream)
    stream.synchronize()
    _same(_results(*out), exp[:4], "top-k on a caller's stream")
    _same([sc.cpu().numpy()], [exp_sc], "scores on a caller's stream")


def test_inverted_slice_is_an_empty_sequence_in_the_device_form(shape):
    st = shape
    rows = rc.unique_lists(st.n, (300,), 97)[0]
    lims = np.array([0, 100, 40, 40, 300, 290], np.uint64)          # queries 1 and 4: inverted; query 2: empty
    lists = [rows[0:100], rows[:0], rows[:0], rows[40:300], rows[:0]]
    for k in (10, 300):
        got = rows_device(st.s, (lims, rows), st.queries, k, metric=st.metric)
        _same(got, rr.topk_batch(lists, st.indexed, st.d, k)[:4], f"k={k}")
        assert got[2].tolist() == [min(k, 100), 0, 0, min(k, 260), 0] and got[3].tolist() == [100, 0, 0, 260, 0]
    with pytest.raises(st.pqv.PqvError, match="lims must not decrease"):
        st.s.topk_rows(st.queries, 10, (lims, rows), metric=st.metric)
    with pytest.raises(st.pqv.PqvError, match="lims must not decrease"):
        st.s.score_rows(st.queries, (lims, rows), metric=st.metric)


def test_refusals_that_need_a_device_object(pqv, oracle):
    st = shape_setup(pqv, oracle, "1500x30")
    lists = rc.unique_lists(st.n, rc.LENS_A, 99)
    other = pqv.Searcher(st.index, st.corpus)
    om = other.row_mask(np.ones(st.n, bool))
    for call in (lambda: st.s.topk_rows(st.queries, 10, lists, mask=om), lambda: rows_device(st.s, lists, st.queries, 10, mask=om),
                 lambda: st.s.score_rows(st.queries, lists, mask=om), lambda: score_device(st.s, lists, st.queries, mask=om)):
        with pytest.raises(pqv.PqvError, match="row mask belongs to another searcher"):
            call()
    om.close()
    other.close()
    # k beyond the kernels' lists: both forms refuse, there is no host fallback
    for call in (lambda k: st.s.topk_rows(st.queries, k, lists), lambda k: rows_device(st.s, lists, st.queries, k)):
        with pytest.raises(pqv.PqvError, match="pqv_topk_rows takes k <= 1024") as e:
            call(1025)
        assert e.value.code == pqv._ffi.PQV_ERR_UNSUPPORTED
        with pytest.raises(pqv.PqvError, match="k must be > 0"):
            call(0)
    with pytest.raises(pqv.PqvError, match="Query dimension mismatch: expected 30, got 29"):
        st.s.topk_rows(st.queries[:, :29], 10, lists)
    with pytest.raises(pqv.PqvError, match="Query dimension mismatch: expected 30, got 29"):
        st.s.score_rows(st.queries[:, :29], lists)
    with pytest.raises(pqv.PqvError, match="unknown metric"):
        st.s.topk_rows(st.queries, 10, lists, metric=9)
    assert st.s.topk_rows(st.queries[:0], 10, [])[0].shape == (0, 10)
    assert st.s.score_rows(st.queries[:0], [])[1].shape == (0,)
    # table searchers are refused
    t = pqv.TableSearcher([st.index], st.corpus, [0])
    for call, text in ((lambda: t.topk_rows(st.queries, 10, lists), "pqv_topk_rows does not take table searchers"),
                       (lambda: rows_device(t, lists, st.queries, 10), "pqv_topk_rows does not take table searchers"),
                       (lambda: t.score_rows(st.queries, lists), "pqv_score_rows does not take table searchers"),
                       (lambda: score_device(t, lists, st.queries), "pqv_score_rows does not take table searchers")):
        with pytest.raises(pqv.PqvError, match=text) as e:
            call()
        assert e.value.code == pqv._ffi.PQV_ERR_UNSUPPORTED
    t.close()
