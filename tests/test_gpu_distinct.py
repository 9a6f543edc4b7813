"""Distinct top-k on the GPU (pqv_topk_distinct / pqv_topk_distinct_device): the nearest row of each of the k nearest groups.

The yardstick everywhere is the same searcher's EXISTING range search: range_search(q, +inf, nprobe, sqrt_out=False, mask=key
validity AND shared mask) returns the considered rows sorted by (d2, position); numpy keeps the first row of every key value and
cuts to k.  Rows, distance bits, group keys, n_found and n_candidates must be equal, on the host and the device form.
tests/distinct_ref.py over the oracle's candidates is a second opinion."""
import numpy as np
import pytest

import distinct_ref
from range_oracle import l2_chain
from test_gpu_mask import SHAPES, Setup, _bits

pytestmark = pytest.mark.gpu

EMPTY = 0xFFFFFFFF
KS = (1, 5, 64, 65, 200)


def _device(s, q, k, nprobe, keys, mask=None, metric=0, max_candidates=0, sqrt_out=False):
    """topk_distinct_device -> (rows, dist, group keys, n_found, n_candidates); the outputs start as garbage"""
    import torch
    dev = torch.device("cuda", 0)
    q_t = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(dev)
    nq = len(q)
    r_t = torch.full((nq, k), 5, dtype=torch.int32, device=dev)
    d_t = torch.full((nq, k), -1.0, dtype=torch.float32, device=dev)
    g_t = torch.full((nq, k), 77, dtype=torch.int64, device=dev)
    nf_t = torch.full((nq,), 9, dtype=torch.int32, device=dev)
    nc_t = torch.full((nq,), 9, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    s.topk_distinct_device(q_t.data_ptr(), nq, k, nprobe, keys, r_t.data_ptr(), d_t.data_ptr(), g_t.data_ptr(), nf_t.data_ptr(),
                           nc_t.data_ptr(), mask=mask, max_candidates=max_candidates, metric=metric, sqrt_out=sqrt_out)
    torch.cuda.synchronize()
    return (r_t.cpu().numpy().view(np.uint32), d_t.cpu().numpy(), g_t.cpu().numpy(), nf_t.cpu().numpy().astype(np.uint32),
            nc_t.cpu().numpy().astype(np.uint64))


class Distinct:
    """A group column over a searcher's rows, its RowKeys, the optional shared mask, and the yardstick's mask (validity AND shared)."""

    def __init__(self, pqv, s, n_rows, values, valid=None, shared=None):
        self.s, self.values, self.valid, self.shared = s, values, valid, shared
        col = pqv.Column.upload(values, valid, device=0)
        self.keys = s.row_keys(col)
        col.close()
        self.shared_mask = s.row_mask(shared) if shared is not None else None
        self.allowed = distinct_ref.considered_mask(n_rows, valid, shared)
        self.ymask = s.row_mask(self.allowed)

    def close(self):
        self.ymask.close()
        if self.shared_mask is not None:
            self.shared_mask.close()
        self.keys.close()

    def yardstick(self, q, k, nprobe, metric=0, max_candidates=0):
        lims, rows, dist, _, nc = self.s.range_search(q, np.inf, nprobe, sqrt_out=False, mask=self.ymask, metric=metric,
                                                      max_candidates=max_candidates)
        nq = len(q)
        o_r = np.full((nq, k), EMPTY, np.uint32); o_d = np.full((nq, k), np.inf, np.float32)
        o_g = np.zeros((nq, k), np.int64); o_n = np.zeros(nq, np.uint32)
        for i in range(nq):
            a, b = int(lims[i]), int(lims[i + 1])
            r, d, g = distinct_ref.dedup_sorted(rows[a:b], dist[a:b], self.values, k)
            o_r[i, :len(r)], o_d[i, :len(r)], o_g[i, :len(r)], o_n[i] = r, d, g, len(r)
        return o_r, o_d, o_g, o_n, nc

    def host(self, q, k, nprobe, metric=0, max_candidates=0):
        return self.s.topk_distinct(q, k, nprobe, self.keys, mask=self.shared_mask, metric=metric, max_candidates=max_candidates,
                                    sqrt_out=False)

    def device(self, q, k, nprobe, metric=0, max_candidates=0):
        return _device(self.s, q, k, nprobe, self.keys, mask=self.shared_mask, metric=metric, max_candidates=max_candidates)

    def check(self, q, k, nprobe, what="", forms=("host", "device"), **kw):
        exp = self.yardstick(q, k, nprobe, **kw)
        for form in forms:
            got = getattr(self, form)(q, k, nprobe, **kw)
            w = f"{form} k={k} nprobe={nprobe} {what}"
            assert (got[3] == exp[3]).all(), "n_found " + w
            assert (got[0] == exp[0]).all(), "rows " + w
            assert (_bits(got[1]) == _bits(exp[1])).all(), "distance bits " + w
            assert (got[2] == exp[2]).all(), "group keys " + w
            assert (got[4] == exp[4]).all(), "n_candidates " + w
        return exp


@pytest.fixture(scope="module", params=list(SHAPES))
def shape(request, pqv, oracle):
    c = SHAPES[request.param]
    st = Setup(pqv, oracle, c["n"], c["dim"], c["kc"], seed=11 + c["dim"])
    st.metric = c["metric"]
    return st


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_every_shape_equals_the_deduplicated_range_search(pqv, shape, dtype):
    """Case 1: about 16 rows per key -- a group's members fall into the same tile, other waves, other blocks and other lists."""
    st = shape
    values = st.rng.integers(0, st.n // 16, st.n).astype(dtype)
    d = Distinct(pqv, st.s, st.n, values)
    try:
        for nprobe in (1, 3, st.kc):
            for k in KS:
                exp = d.check(st.queries, k, nprobe, metric=st.metric)
                assert (exp[3] == np.minimum(k, [len(np.unique(values[st.oidx.candidate_rows(q, nprobe)])) for q in st.queries])).all()
        # the second opinion: the restatement over the oracle's candidates
        for q in st.queries[:2]:
            r, d2, g, nc, _ = distinct_ref.distinct_topk(st.oidx.candidate_rows(q, 3), values, None, None, st.data, q, 65, metric=st.metric)
            got = d.host(q.reshape(1, -1), 65, 3, metric=st.metric)
            n = int(got[3][0])
            assert n == len(r) and (got[0][0, :n] == r).all() and (_bits(got[1][0, :n]) == _bits(d2)).all() and (got[2][0, :n] == g).all()
            assert got[4][0] == nc
    finally:
        d.close()


def test_integer_data_ties_follow_d2_then_position(pqv, oracle):
    """Case 2: whole distance classes tie: the representative and the rank follow (d2, position)."""
    st = Setup(pqv, oracle, 3000, 8, 6, seed=4, integer=True)
    q = np.random.default_rng(2).integers(0, 3, (9, 8)).astype(np.float32)
    d = Distinct(pqv, st.s, st.n, st.rng.integers(0, st.n // 16, st.n).astype(np.int64))
    try:
        for k, nprobe in ((5, 2), (100, st.kc), (200, 3)):
            exp = d.check(q, k, nprobe)
            if k >= 100:     # (d2 is an integer <= 32: a hundred entries must tie)
                assert (exp[3] >= 100).any()
                assert all(len(np.unique(_bits(exp[1][i, :int(exp[3][i])]))) < int(exp[3][i]) for i in range(len(q)) if exp[3][i] >= 100)
        r, d2, g, _, _ = distinct_ref.distinct_topk(st.oidx.candidate_rows(q[0], 2), d.values, None, None, st.data, q[0], 100)
        got = d.host(q[:1], 100, 2)
        assert (got[0][0, :len(r)] == r).all() and (_bits(got[1][0, :len(r)]) == _bits(d2)).all() and (got[2][0, :len(r)] == g).all()
    finally:
        d.close()


@pytest.mark.parametrize("kind", ["high-word", "low-word", "negative"])
def test_wide_keys_are_compared_in_full(pqv, oracle, kind):
    """Case 3: I64 keys that differ only in the high word / only in the low word, and negative keys: a half-width compare merges
    groups that are different."""
    st = Setup(pqv, oracle, 4096, 128, 8, seed=23)
    g = st.rng.integers(0, st.n // 16, st.n).astype(np.int64)
    values = {"high-word": (g << 32) + 7, "low-word": (5 << 32) + g, "negative": -(g * (2 ** 32 + 12345)) - 1}[kind]
    d = Distinct(pqv, st.s, st.n, values)
    try:
        for k in (5, 65):
            d.check(st.queries, k, 3, kind)
    finally:
        d.close()
    if kind == "negative":       # ... and negative I32 keys come back sign-extended
        d = Distinct(pqv, st.s, st.n, (-g - 1).astype(np.int32))
        try:
            exp = d.check(st.queries, 65, 3, "negative i32")
            assert (exp[2][exp[0] != EMPTY] < 0).all()
        finally:
            d.close()


def test_all_keys_distinct_is_the_masked_top_k(pqv, shape):
    """Case 4: bit-equal to topk_device under an all-ones mask (rows, distances, n_found)."""
    from test_gpu_mask import _device as masked_device
    st = shape
    d = Distinct(pqv, st.s, st.n, st.rng.permutation(st.n).astype(np.int64) - st.n // 2)
    ones = st.s.row_mask(np.ones(st.n, bool))
    try:
        for k, nprobe in ((1, 1), (64, 3), (200, st.kc)):
            exp = masked_device(st.s, st.queries, k, nprobe, False, mask=ones, metric=st.metric)
            for got in (d.host(st.queries, k, nprobe, metric=st.metric), d.device(st.queries, k, nprobe, metric=st.metric)):
                assert (got[0] == exp[0]).all() and (_bits(got[1]) == _bits(exp[1])).all() and (got[3] == exp[2]).all()
                assert (got[4] == exp[3]).all()
                assert (got[2] == d.values[got[0].astype(np.int64)]).all()
    finally:
        ones.close(); d.close()


def test_all_keys_equal_is_the_nearest_row(pqv, shape):
    """Case 5."""
    st = shape
    d = Distinct(pqv, st.s, st.n, np.full(st.n, -42, np.int32))
    try:
        for k in (1, 65):
            exp = d.check(st.queries, k, 3, metric=st.metric)
            near = st.s.topk(st.queries, 1, 3, metric=st.metric, sqrt_out=False)
            assert (exp[3] == 1).all() and (exp[0][:, 0] == near[0][:, 0]).all() and (_bits(exp[1][:, 0]) == _bits(near[1][:, 0])).all()
            assert (exp[2][:, 0] == -42).all() and (exp[0][:, 1:] == EMPTY).all()
    finally:
        d.close()


@pytest.mark.parametrize("order", ["descending", "ascending"])
def test_lists_ordered_by_distance(pqv, oracle, order):
    """Case 6: every list sorted by the distance to query 0, descending (every considered row replaces its group's entry) and
    ascending (none does)."""
    n, dim, kc, seed = 4096, 128, 8, 31
    rng = np.random.default_rng(seed)            # (Setup draws its rows and queries first, in this order)
    data = rng.random((n, dim), dtype=np.float32)
    q0 = rng.random((5, dim), dtype=np.float32)[0]

    def reorder(lists):
        out = []
        for l in lists:
            l = np.asarray(l, np.uint32)
            d2 = l2_chain(data[l.astype(np.int64)], q0, 0)
            o = np.argsort(d2, kind="stable")
            out.append(l[o[::-1]] if order == "descending" else l[o])
        return out
    st = Setup(pqv, oracle, n, dim, kc, seed=seed, lists=reorder)
    assert (st.data == data).all() and (st.queries[0] == q0).all()
    d = Distinct(pqv, st.s, st.n, st.rng.integers(0, st.n // 16, st.n).astype(np.int64))
    try:
        for k in (5, 65, 200):
            d.check(st.queries, k, 3, order)
    finally:
        d.close()


def test_null_keys_and_shared_masks(pqv, shape):
    """Case 7: about 30 % NULL keys, a shared mask with p = 0.1, both; a mask that leaves fewer than k groups; one that leaves none."""
    st = shape
    values = st.rng.integers(0, st.n // 16, st.n).astype(np.int32)
    valid = (st.rng.random(st.n) >= 0.3).astype(np.uint8)
    shared = st.rng.random(st.n) < 0.1
    for v, m in ((valid, None), (None, shared), (valid, shared)):
        d = Distinct(pqv, st.s, st.n, values, v, m)
        try:
            for k in (5, 65):
                exp = d.check(st.queries, k, 3, metric=st.metric)
                found = exp[0][exp[0] != EMPTY].astype(np.int64)
                assert d.allowed[found].all()                     # no NULL-key row, no masked row
        finally:
            d.close()
    # fewer than k groups: rows of three key values only
    few = np.isin(values, [1, 2, 3]) & (valid != 0)
    d = Distinct(pqv, st.s, st.n, values, valid, few)
    try:
        exp = d.check(st.queries, 65, st.kc, metric=st.metric)
        assert (exp[3] <= 3).all() and exp[3].max() > 0
        for got in (d.host(st.queries, 65, st.kc, metric=st.metric), d.device(st.queries, 65, st.kc, metric=st.metric)):
            for i, nf in enumerate(got[3]):
                assert (got[0][i, nf:] == EMPTY).all() and np.isposinf(got[1][i, nf:]).all() and (got[2][i, nf:] == 0).all()
    finally:
        d.close()
    d = Distinct(pqv, st.s, st.n, values, valid, np.zeros(st.n, bool))
    try:
        exp = d.check(st.queries, 5, 3, metric=st.metric)
        assert (exp[3] == 0).all() and (exp[0] == EMPTY).all()
    finally:
        d.close()
    # every key NULL, no mask
    d = Distinct(pqv, st.s, st.n, values, np.zeros(st.n, np.uint8))
    try:
        assert (d.check(st.queries, 5, 3, metric=st.metric)[3] == 0).all()
    finally:
        d.close()


@pytest.mark.parametrize("name", ["4096x128", "1500x30"])
def test_max_candidates_cuts_before_the_groups(pqv, oracle, name):
    """Case 8: the cap falls inside the second probed list."""
    c = SHAPES[name]
    st = Setup(pqv, oracle, c["n"], c["dim"], c["kc"], seed=21)
    values = st.rng.integers(0, st.n // 16, st.n).astype(np.int64)
    valid = (st.rng.random(st.n) >= 0.3).astype(np.uint8)
    d = Distinct(pqv, st.s, st.n, values, valid)
    try:
        for q in st.queries[:3]:
            first = len(st.lists[int(st.oidx.find_closest_centroids(q, 1)[0])])
            for cap in (first + 100, 37):
                q1 = q.reshape(1, -1)
                exp = d.check(q1, 10, 3, f"cap={cap}", max_candidates=cap)
                r, d2, g, nc, _ = distinct_ref.distinct_topk(st.oidx.candidate_rows(q, 3), values, valid, None, st.data, q, 10,
                                                             max_candidates=cap)
                n = int(exp[3][0])
                assert n == len(r) and (exp[0][0, :n] == r).all() and (_bits(exp[1][0, :n]) == _bits(d2)).all() and exp[4][0] == nc
    finally:
        d.close()


def test_two_file_table_with_the_round_robin_cap(pqv, oracle):
    """Case 9."""
    from test_gpu_table import Table
    from test_gpu_table_cap import _selected
    rng = np.random.default_rng(12)
    t = Table(pqv, oracle, rng, [900, 1400], [4, 6], 32, gap=5, flags=pqv.PQV_TABLE_CAP_ROUND_ROBIN)
    n = len(t.data)
    values = rng.integers(0, n // 16, n).astype(np.int64)
    shared = rng.random(n) < 0.5
    d = Distinct(pqv, t.s, n, values, None, shared)
    queries = rng.random((4, 32), dtype=np.float32)
    try:
        for nprobe in (1, 2):
            for cap in (0, 500):
                d.check(queries, 10, nprobe, f"cap={cap}", max_candidates=cap)
                d.check(queries, 65, nprobe, f"cap={cap}", max_candidates=cap)
                q = queries[0]
                cand = t.cand(q, nprobe)
                sel = _selected(t, oracle, q, nprobe, cap)[0] if cap else cand
                r, d2, g, _, _ = distinct_ref.distinct_topk(sel, values, None, shared, t.data, q, 10)
                got = d.host(q.reshape(1, -1), 10, nprobe, max_candidates=cap)
                assert int(got[3][0]) == len(r) and (got[0][0, :len(r)] == r).all() and (got[2][0, :len(r)] == g).all()
                assert got[4][0] == len(cand)
    finally:
        d.close()


def test_cosine(pqv, oracle):
    """Case 10: PQV_COSINE through the cosine layout: the halved distances of the cosine range search, deduplicated."""
    st = Setup(pqv, oracle, 2048, 256, 4, seed=33)
    d = Distinct(pqv, st.s, st.n, st.rng.integers(0, st.n // 16, st.n).astype(np.int32), (st.rng.random(st.n) >= 0.3).astype(np.uint8))
    try:
        for k in (5, 65):
            d.check(st.queries, k, 2, "cosine", metric=pqv.PQV_COSINE)
    finally:
        d.close()


def test_counters(pqv, oracle):
    """Case 11: embeddings_fetched advances by the considered rows, candidate_rows by the uncapped total."""
    import mask_ref
    st = Setup(pqv, oracle, 4096, 128, 8, seed=17)
    values = st.rng.integers(0, st.n // 16, st.n).astype(np.int64)
    valid = (st.rng.random(st.n) >= 0.3).astype(np.uint8)
    d = Distinct(pqv, st.s, st.n, values, valid, st.rng.random(st.n) < 0.5)
    cap = 700
    cons = sum(len(mask_ref.considered(st.oidx.candidate_rows(q, 3), d.allowed, cap)[0]) for q in st.queries)
    tot = sum(len(st.oidx.candidate_rows(q, 3)) for q in st.queries)
    try:
        for call in (d.host, d.device):
            before = st.s.counters()
            call(st.queries, 10, 3, max_candidates=cap)
            after = st.s.counters()
            assert after["embeddings_fetched"] - before["embeddings_fetched"] == cons
            assert after["candidate_rows"] - before["candidate_rows"] == tot
            assert after["queries"] - before["queries"] == len(st.queries)
    finally:
        d.close()


def test_beyond_the_kernel_lists(pqv, oracle):
    """Case 12: k = 1100 (host form: the range machinery and a host pass; device form: PQV_ERR_UNSUPPORTED), and 1100 probed lists."""
    st = Setup(pqv, oracle, 4096, 128, 8, seed=35)
    d = Distinct(pqv, st.s, st.n, st.rng.permutation(st.n).astype(np.int64))
    try:
        exp = d.check(st.queries[:2], 1100, st.kc, forms=("host",))
        assert (exp[3] == 1100).all()
        with pytest.raises(pqv.PqvError) as e:
            d.device(st.queries[:1], 1100, st.kc)
        assert e.value.code == -5
    finally:
        d.close()
    st = Setup(pqv, oracle, 2200, 8, 1100, seed=15)
    d = Distinct(pqv, st.s, st.n, st.rng.integers(0, st.n // 16, st.n).astype(np.int32), (st.rng.random(st.n) >= 0.3).astype(np.uint8))
    try:
        before = st.s.counters()
        exp = d.check(st.queries[:2], 10, 1100, forms=("host",))
        after = st.s.counters()
        assert (exp[3] == 10).all()
        r, d2, g, nc, ncons = distinct_ref.distinct_topk(st.oidx.candidate_rows(st.queries[0], 1100), d.values, d.valid, None, st.data,
                                                         st.queries[0], 10)
        assert (exp[0][0] == r).all() and (_bits(exp[1][0]) == _bits(d2)).all() and (exp[2][0] == g).all() and exp[4][0] == nc
        with pytest.raises(pqv.PqvError) as e:
            d.device(st.queries[:1], 10, 1100)
        assert e.value.code == -5
        # (the yardstick's range search and the distinct call count the same rows: twice the considered rows of the two queries)
        cons = sum(int(d.allowed[st.oidx.candidate_rows(q, 1100)].sum()) for q in st.queries[:2])
        assert after["embeddings_fetched"] - before["embeddings_fetched"] == 2 * cons
    finally:
        d.close()


def test_errors_that_need_a_searcher(pqv, oracle):
    """Case 13."""
    st = Setup(pqv, oracle, 1500, 30, 6, seed=19)
    other = pqv.Searcher(pqv.Index.from_parts(30, st.centroids, st.lists), st.corpus)
    d = Distinct(pqv, st.s, st.n, np.arange(st.n, dtype=np.int32), None, np.ones(st.n, bool))
    foreign_mask = other.row_mask(np.ones(st.n, bool))
    try:
        for call in (lambda: other.topk_distinct(st.queries, 5, 2, d.keys), lambda: _device(other, st.queries, 5, 2, d.keys)):
            with pytest.raises(pqv.PqvError, match="row keys belong to another searcher") as e:
                call()
            assert e.value.code == -1
        for call in (lambda: st.s.topk_distinct(st.queries, 5, 2, d.keys, mask=foreign_mask),
                     lambda: _device(st.s, st.queries, 5, 2, d.keys, mask=foreign_mask)):
            with pytest.raises(pqv.PqvError, match="row mask belongs to another searcher") as e:
                call()
            assert e.value.code == -1
        with pytest.raises(pqv.PqvError, match="k must be > 0"):
            st.s.topk_distinct(st.queries, 0, 2, d.keys)
        with pytest.raises(pqv.PqvError, match="nprobe must be > 0"):
            st.s.topk_distinct(st.queries, 5, 0, d.keys)
        with pytest.raises(pqv.PqvError, match="Query dimension mismatch"):
            st.s.topk_distinct(st.queries[:, :7], 5, 2, d.keys)
        # the optional outputs may be NULL
        import torch
        dev = torch.device("cuda", 0)
        q_t = torch.from_numpy(st.queries).to(dev)
        r_t = torch.zeros((5, 5), dtype=torch.int32, device=dev); d_t = torch.zeros((5, 5), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        st.s.topk_distinct_device(q_t.data_ptr(), 5, 5, 2, d.keys, r_t.data_ptr(), d_t.data_ptr(), sqrt_out=False)
        torch.cuda.synchronize()
        exp = d.yardstick(st.queries, 5, 2)
        assert (r_t.cpu().numpy().view(np.uint32) == exp[0]).all() and (_bits(d_t.cpu().numpy()) == _bits(exp[1])).all()
    finally:
        foreign_mask.close(); d.close(); other.close()


def test_builders(pqv, tmp_path):
    """Case 14: .distinct_on("doc") on a written Parquet file with an int64 doc column, with and without .where(), and on a
    two-file table; against the yardstick on the same resident searcher."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    rng = np.random.default_rng(41)
    paths, docs = [], []
    for f, n in enumerate((300, 200)):
        vec = rng.random((n, 8), dtype=np.float32)
        doc = rng.integers(-20, 20, n).astype(np.int64) * (2 ** 33 + 1)
        path = str(tmp_path / f"f{f}.parquet")
        pq.write_table(pa.table({"id": pa.array(range(n), type=pa.int32()), "doc": pa.array(doc, type=pa.int64()),
                                 "vec": pa.array(vec.tolist(), type=pa.list_(pa.float32()))}), path)
        pqv.IndexBuilder(path, "vec").n_clusters(4).build_inplace()
        paths.append(path); docs.append(doc)
    query = rng.random(8, dtype=np.float32)

    def expect(s, column, allowed, k, nprobe):
        m = s.row_mask(allowed)
        try:
            _, rows, dist, _, _ = s.range_search(query, np.inf, nprobe, mask=m)
        finally:
            m.close()
        return distinct_ref.dedup_sorted(rows, dist, column, k)

    s = pqv.searcher_for_parquet(paths[0])
    for where in (False, True):
        b = pqv.TopkBuilder(paths[0], query).k(7).nprobe(3).distinct_on("doc")
        if where:
            b = b.where(pqv.col("id") >= 2)
        res = b.search()
        r, dd, g = expect(s, docs[0], np.arange(300) >= (2 if where else 0), 7, 3)
        assert len(res) == 7 and isinstance(res[0], pqv.DistinctSearchResult)
        assert [x.row_idx for x in res] == r.tolist() and [x.key for x in res] == g.tolist()
        assert [np.float32(x.distance) for x in res] == dd.tolist()
    assert "doc" in s.columns
    # a Searcher source: the attached column by name, or a RowKeys
    keys = s.row_keys("doc")
    by_keys = pqv.TopkBuilder(s, query).k(7).nprobe(3).distinct_on(keys).metric(pqv.PQV_L2SQ_REF4).search()
    by_name = pqv.TopkBuilder(s, query).k(7).nprobe(3).distinct_on("doc").search()
    keys.close()
    r, dd, g = expect(s, docs[0], np.ones(300, bool), 7, 3)
    assert [x.row_idx for x in by_keys] == [x.row_idx for x in by_name] == r.tolist()
    # the table
    ts = pqv.searcher_for_parquet_files(paths)
    doc_all = np.concatenate(docs)
    for where in (False, True):
        b = pqv.TableTopkBuilder(paths, query).k(9).nprobe(2).distinct_on("doc")
        if where:
            b = b.where(pqv.col("id") >= 2)
        res = b.search()
        allowed = np.concatenate([np.arange(300) >= 2, np.arange(200) >= 2]) if where else np.ones(500, bool)
        r, dd, g = expect(ts, doc_all, allowed, 9, 2)
        f, local = ts.split_rows(r)
        assert [x.path for x in res] == [paths[int(i)] for i in f] and [x.row_idx for x in res] == local.tolist()
        assert [x.key for x in res] == g.tolist() and [np.float32(x.distance) for x in res] == dd.tolist()
        assert len(set(x.key for x in res)) == len(res) == 9


# ---- host sub-batches: one call of more queries than the lane's scratch bound lets one pass hold ---------------------------------
def host_batch(kc, dim, k, m):
    """The queries one sub-batch of a host distinct (m = 1) / grouped call holds at 4096 x 128 over all kc = 8 lists: the per-query
    scratch of the grouped branch of pqv_topk_impl (csrc/api.cpp) against its 1 GiB bound, restated from the code."""
    n_part_rr = kc * 1 * 4                  # exact stream, >= 8192 (query, list) pairs: one block of four waves per list
    n_part_probe, probe_kpart = 4, 64       # 8 centroids: one probe block of four waves; probe_rows_kernel's 64 unsorted entries
    km = k * m
    per_query = (n_part_rr * max(k * 20, km * 16 + 4 if m > 1 else 0) + n_part_probe * probe_kpart * 12 + kc * 32 + (dim + dim) * 4 +
                 20 * k + (8 * km if m > 1 else 0) + 16)
    return (1 << 30) // per_query


# the per-query filters of the filtered runs: six patterns cycle over the queries, so the second sub-batch is right only if it got
# its own slice of the arrays and IN lims rebased to it (sets of 300, 0, 1, 2, 65 and 7 values)
SUB_FILTERS = {
    "eq": [3, 0, 99, 63, 17, 40],                                                         # (99: no row's key)
    "range": ([0, 2, 5, 63, -100, -(2 ** 63)], [7, 40, 4, 63, 0, 2 ** 63 - 1]),           # (5 > 4: nothing; the last: every key)
    "in": [list(range(-150, 150)), [], [5], [-3, 17], list(range(0, 130, 2)), [1, 2, 3, 60, 61, 62, 1000]],
}


def check_host_sub_batches(pqv, oracle, m, filt):
    """m None: topk_distinct, else topk_grouped with group_size m; filt: None or a key of SUB_FILTERS.  The call of
    nq = batch + batch // 2 queries is compared (a) with the deduplicated range search -- the yardstick of this file, under the
    mask M_q of the query's filter pattern -- for the first 64 queries, the 64 on each side of q0 = batch and the last 64, and (b)
    for every query with the concatenation of calls of at most 1000 queries, every output bit for bit."""
    import distinct_filter_ref as fref
    import grouped_ref
    c = SHAPES["4096x128"]
    st = Setup(pqv, oracle, c["n"], c["dim"], c["kc"], seed=71)
    k, nprobe = 300, st.kc
    batch = host_batch(st.kc, c["dim"], k, m or 1)
    assert 1000 < batch < 8000
    nq = batch + batch // 2                 # (the second sub-batch starts in the middle of the call)
    rng = np.random.default_rng(72)
    q = rng.random((nq, c["dim"]), dtype=np.float32)
    values = rng.integers(0, 1024, st.n).astype(np.int64)
    valid = (rng.random(st.n) >= 0.1).astype(np.uint8)
    fvalues = rng.integers(0, 64, st.n).astype(np.int32)
    fvalid = (rng.random(st.n) >= 0.1).astype(np.uint8)
    col = pqv.Column.upload(values, valid, device=0)
    gkeys = st.s.row_keys(col)
    col.close()
    col = pqv.Column.upload(fvalues, fvalid, device=0)
    fkeys = st.s.row_keys(col)
    col.close()
    which = np.arange(nq) % 6
    kind, pat = (getattr(fref, filt.upper()), SUB_FILTERS[filt]) if filt else (None, None)

    def spec(idx):      # the filter of the queries idx, as distinct_filter_ref states one
        if kind == fref.RANGE:
            return [pat[0][which[i]] for i in idx], [pat[1][which[i]] for i in idx]
        return [pat[which[i]] for i in idx]

    def call(a, b):
        kw = dict(sqrt_out=False)
        if filt:
            kw.update(filter_keys=fkeys, **fref.call_kw(kind, spec(range(a, b))))
        if m is None:
            return st.s.topk_distinct(q[a:b], k, nprobe, gkeys, **kw)
        return st.s.topk_grouped(q[a:b], k, m, nprobe, gkeys, **kw)

    got = call(0, nq)
    names = ("rows", "dist", "group_key") + (() if m is None else ("group_rows",)) + ("n_found", "n_candidates")
    assert len(got) == len(names)
    # (b) the same queries in calls of at most 1000
    small = [call(a, min(a + 1000, nq)) for a in range(0, nq, 1000)]
    for j, name in enumerate(names):
        whole, parts = np.ascontiguousarray(got[j]), np.concatenate([p[j] for p in small])
        assert whole.shape == parts.shape and (whole.view(np.uint8) == parts.view(np.uint8)).all(), f"{name}: one call != smaller calls"
    # (a) the yardstick around both ends and the cut
    sel = np.concatenate([np.arange(0, 64), np.arange(batch - 64, batch + 64), np.arange(nq - 64, nq)])
    n_full = n_some = 0
    for w in range(6 if filt else 1):
        idx = sel[which[sel] == w] if filt else sel
        allowed = distinct_ref.considered_mask(st.n, valid)
        if filt:
            allowed = allowed & fref.allowed(fvalues, fvalid, kind, spec([w]), 0)
        ymask = st.s.row_mask(allowed)
        lims, rows, dist, _, nc = st.s.range_search(q[idx], np.inf, nprobe, sqrt_out=False, mask=ymask)
        ymask.close()
        for j, i in enumerate(idx):
            a, b = int(lims[j]), int(lims[j + 1])
            what = f"query {i} (filter pattern {w})"
            if m is None:
                r, d, g = distinct_ref.dedup_sorted(rows[a:b], dist[a:b], values, k)
                n = len(r)
                assert got[3][i] == n, "n_found of " + what
                assert (got[0][i, :n] == r).all() and (got[0][i, n:] == EMPTY).all(), "rows of " + what
                assert (_bits(got[1][i, :n]) == _bits(d)).all() and np.isposinf(got[1][i, n:]).all(), "distance bits of " + what
                assert (got[2][i, :n] == g).all() and (got[2][i, n:] == 0).all(), "group keys of " + what
            else:
                r, d, g, cnt, n = grouped_ref.group_sorted(rows[a:b], dist[a:b], values, k, m)
                assert got[4][i] == n, "n_found of " + what
                assert (got[0][i] == r).all() and (_bits(got[1][i]) == _bits(d)).all(), "rows / distance bits of " + what
                assert (got[2][i] == g).all() and (got[3][i] == cnt).all(), "group keys / group_rows of " + what
            assert got[-1][i] == nc[j], "n_candidates of " + what
            n_full += n == k
            n_some += n > 0
    if not filt:
        assert n_full == len(sel)           # (about a thousand valid key values in the probed lists: every query finds k groups)
    elif filt != "eq":
        assert n_full > 0                   # (the full range and the 300-value set pass every filter key)
    assert n_some > len(sel) // 2
    fkeys.close()
    gkeys.close()


@pytest.mark.parametrize("filt", [None, "eq", "range", "in"])
def test_host_sub_batches(pqv, oracle, filt):
    """One host call of more queries than one sub-batch holds (k = 300, 4096 x 128, all 8 lists): the second sub-batch's results,
    group keys and counts land at their offsets, and its filter slice is its own."""
    check_host_sub_batches(pqv, oracle, None, filt)
