"""Distinct / grouped top-k under a per-query key filter on the GPU (pqv_topk_distinct_filtered*, pqv_topk_grouped_filtered*).

The yardstick is the same searcher's EXISTING calls: for every query q the test builds M_q = filter validity AND F_q(filter key) AND
shared mask in numpy (tests/key_filter_ref.py), makes row_mask(M_q), and runs the single-query topk_distinct / topk_grouped with
mask=.  Rows, distance bits, group keys, group_rows, n_found and n_candidates must be equal, for the host and the device form
(device-resident filter arrays, outputs that start as garbage).  No tolerance anywhere.  tests/distinct_filter_ref.py over the
oracle's candidates is the second opinion.  The inputs' non-vacuity is checked without a GPU by tests/test_distinct_filter_host.py."""
import numpy as np
import pytest

import distinct_filter_cases as cases
import distinct_filter_ref as ref
from distinct_filter_ref import EQ, IN, RANGE
from test_gpu_mask import SHAPES, Setup, _bits

pytestmark = pytest.mark.gpu

EMPTY = 0xFFFFFFFF
I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1


def _filter_tensors(kind, spec, dev):
    """the descriptor's arrays on the device -> (keywords of the _device calls, the tensors to keep alive)"""
    import torch
    k, a, b = ref.descriptor(kind, spec)
    a_t = torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev)
    if kind == EQ:
        return {"query_keys": a_t.data_ptr()}, (a_t,)
    b_t = torch.from_numpy(np.ascontiguousarray(b if len(b) else np.zeros(1, np.int64))).to(dev)
    name = "query_key_ranges" if kind == RANGE else "query_key_sets"
    return {name: (a_t.data_ptr(), b_t.data_ptr())}, (a_t, b_t)


class Filtered:
    """A group column, a filter column (the same RowKeys object where the arrays are the same object), an optional shared mask, and
    the per-query yardstick masks M_q, made once per (filter, query) and shared by every k, nprobe and call checked against them."""

    def __init__(self, pqv, s, n, group, fvalues, gvalid=None, fvalid=None, shared=None):
        self.pqv, self.s, self.n = pqv, s, n
        self.group, self.gvalid, self.fvalues, self.fvalid, self.shared = group, gvalid, fvalues, fvalid, shared
        col = pqv.Column.upload(group, gvalid, device=0)
        self.gkeys = s.row_keys(col)
        col.close()
        if fvalues is group and fvalid is gvalid:
            self.fkeys = self.gkeys
        else:
            col = pqv.Column.upload(fvalues, fvalid, device=0)
            self.fkeys = s.row_keys(col)
            col.close()
        self.shared_mask = s.row_mask(shared) if shared is not None else None
        self._mq, self._yard = {}, {}

    def close(self):
        for m in self._mq.values():
            m.close()
        if self.shared_mask is not None:
            self.shared_mask.close()
        if self.fkeys is not self.gkeys:
            self.fkeys.close()
        self.gkeys.close()

    def allowed(self, kind, spec, qi):
        return ref.allowed(self.fvalues, self.fvalid, kind, spec, qi, self.shared)

    def mq(self, kind, spec, qi):
        key = (kind, repr(spec), qi)
        if key not in self._mq:
            self._mq[key] = self.s.row_mask(self.allowed(kind, spec, qi))
        return self._mq[key]

    # ---- the yardstick: nq single-query calls of the EXISTING entry points under M_q --------------------------------------------
    def yardstick(self, q, kind, spec, k, m, nprobe, metric=0, max_candidates=0):
        key = (q.tobytes(), kind, repr(spec), k, m, nprobe, metric, max_candidates)
        if key not in self._yard:
            out = []
            for i in range(len(q)):
                kw = dict(mask=self.mq(kind, spec, i), metric=metric, max_candidates=max_candidates, sqrt_out=False)
                if m is None:
                    out.append(self.s.topk_distinct(q[i:i + 1], k, nprobe, self.gkeys, **kw))
                else:
                    out.append(self.s.topk_grouped(q[i:i + 1], k, m, nprobe, self.gkeys, **kw))
            self._yard[key] = tuple(np.concatenate([o[j] for o in out]) for j in range(len(out[0])))
        return self._yard[key]

    # ---- the calls under test -------------------------------------------------------------------------------------------------
    def host(self, q, kind, spec, k, m, nprobe, metric=0, max_candidates=0, sqrt_out=False):
        kw = dict(mask=self.shared_mask, metric=metric, max_candidates=max_candidates, sqrt_out=sqrt_out, filter_keys=self.fkeys,
                  **ref.call_kw(kind, spec))
        if m is None:
            return self.s.topk_distinct(q, k, nprobe, self.gkeys, **kw)
        return self.s.topk_grouped(q, k, m, nprobe, self.gkeys, **kw)

    def device(self, q, kind, spec, k, m, nprobe, metric=0, max_candidates=0, sqrt_out=False):
        """the device form: device-resident filter arrays, outputs pre-filled with garbage, ONE synchronise behind the call"""
        import torch
        dev = torch.device("cuda", 0)
        q_t = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(dev)
        nq = len(q)
        fkw, alive = _filter_tensors(kind, spec, dev)
        shape = (nq, k) if m is None else (nq, k, m)
        r_t = torch.full(shape, 5, dtype=torch.int32, device=dev)
        d_t = torch.full(shape, -1.0, dtype=torch.float32, device=dev)
        g_t = torch.full((nq, k), 77, dtype=torch.int64, device=dev)
        c_t = torch.full((nq, k), 99, dtype=torch.int32, device=dev)
        nf_t = torch.full((nq,), 9, dtype=torch.int32, device=dev)
        nc_t = torch.full((nq,), 9, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        kw = dict(mask=self.shared_mask, max_candidates=max_candidates, metric=metric, sqrt_out=sqrt_out, filter_keys=self.fkeys, **fkw)
        if m is None:
            self.s.topk_distinct_device(q_t.data_ptr(), nq, k, nprobe, self.gkeys, r_t.data_ptr(), d_t.data_ptr(), g_t.data_ptr(),
                                        nf_t.data_ptr(), nc_t.data_ptr(), **kw)
        else:
            self.s.topk_grouped_device(q_t.data_ptr(), nq, k, m, nprobe, self.gkeys, r_t.data_ptr(), d_t.data_ptr(), g_t.data_ptr(),
                                       c_t.data_ptr(), nf_t.data_ptr(), nc_t.data_ptr(), **kw)
        torch.cuda.synchronize()
        del alive
        out = [r_t.cpu().numpy().view(np.uint32), d_t.cpu().numpy(), g_t.cpu().numpy()]
        if m is not None:
            out.append(c_t.cpu().numpy().view(np.uint32))
        return tuple(out + [nf_t.cpu().numpy().astype(np.uint32), nc_t.cpu().numpy().astype(np.uint64)])

    def check(self, q, kind, spec, k, m, nprobe, what="", forms=("host", "device"), **kw):
        """m None: the distinct calls, outputs (rows, dist, keys, n_found, n_candidates); else the grouped calls, group_rows behind keys"""
        exp = self.yardstick(q, kind, spec, k, m, nprobe, **kw)
        names = ("rows", "distance bits", "group keys") + (() if m is None else ("group_rows",)) + ("n_found", "n_candidates")
        for form in forms:
            got = getattr(self, form)(q, kind, spec, k, m, nprobe, **kw)
            w = f"{form} kind={kind} k={k} m={m} nprobe={nprobe} {what}"
            assert len(got) == len(exp) == len(names)
            for name, x, y in zip(names, got, exp):
                assert x.shape == y.shape, f"shape of {name} " + w
                if name == "distance bits":
                    x, y = _bits(x), _bits(y)
                assert (np.asarray(x) == np.asarray(y)).all(), f"{name} " + w
        return exp


@pytest.fixture(scope="module", params=list(SHAPES))
def shape(request, pqv, oracle):
    c = SHAPES[request.param]
    st = Setup(pqv, oracle, c["n"], c["dim"], c["kc"], seed=11 + c["dim"])
    st.metric, st.name = c["metric"], request.param
    return st


@pytest.mark.parametrize("dtypes", [(np.int32, np.int32), (np.int64, np.int64), (np.int32, np.int64), (np.int64, np.int32)],
                         ids=["i32-i32", "i64-i64", "f32-g64", "f64-g32"])
@pytest.mark.parametrize("kind", list(cases.KINDS))
def test_every_shape_and_filter_equals_the_masked_twin(pqv, shape, kind, dtypes):
    """Case 1: CG 32 / 64, unaligned + tail, SEQ x EQ / RANGE / IN x column widths; about 8 tenants and 16 rows per doc, docs
    spanning tenants."""
    st = shape
    tenant, doc = cases.columns(st.name, st.n, *dtypes)
    spec, kd = cases.SPECS[kind], cases.KINDS[kind]
    f = Filtered(pqv, st.s, st.n, doc, tenant)
    try:
        for nprobe in (1, 3, st.kc):
            for k in cases.KS:
                exp = f.check(st.queries, kd, spec, k, None, nprobe, metric=st.metric)
            found = exp[0][exp[0] != EMPTY].astype(np.int64)
            assert len(found) and all(f.allowed(kd, spec, i)[exp[0][i][exp[0][i] != EMPTY].astype(np.int64)].all() for i in range(len(st.queries)))
        # the second opinion: the restatement over the oracle's candidates
        for qi in (0, 3):
            q = st.queries[qi]
            r, d2, g, nc, _ = ref.distinct_topk(st.oidx.candidate_rows(q, 3), doc, None, tenant, None, kd, spec, qi, None, st.data, q, 65,
                                                metric=st.metric)
            got = f.host(st.queries, kd, spec, 65, None, 3, metric=st.metric)
            n = int(got[3][qi])
            assert n == len(r) and (got[0][qi, :n] == r).all() and (_bits(got[1][qi, :n]) == _bits(d2)).all() and (got[2][qi, :n] == g).all()
            assert got[4][qi] == nc
    finally:
        f.close()


def test_window_edges(pqv, oracle):
    """Case 2: passing positions at offsets 0, 63 and 64 of a list, at the last position of a wave's range and of a list; an index
    with an empty list and one shorter than 64.  The filter column is 1 at the chosen positions and 0 elsewhere, the query key 1."""
    def reshape(lists):
        lists = [np.asarray(l, np.uint32) for l in lists]
        lists[1] = np.concatenate([lists[1], lists[0]]); lists[0] = lists[0][:0]
        lists[3] = np.concatenate([lists[3], lists[2][10:]]); lists[2] = lists[2][:10]
        return lists
    st = Setup(pqv, oracle, 1500, 30, 6, seed=9, lists=reshape)
    assert len(st.lists[0]) == 0 and len(st.lists[2]) == 10
    doc = st.rng.integers(0, st.n // 4, st.n).astype(np.int32)
    big = max(range(st.kc), key=lambda c: len(st.lists[c]))
    lst, short = st.lists[big].astype(np.int64), st.lists[2].astype(np.int64)
    assert len(lst) > 300
    for pos in ([0], [63], [64], [0, 63, 64], [len(lst) - 1], [255, 256], [63, 127, 191, 255], range(10, 75), range(len(lst))):
        tenant = np.zeros(st.n, np.int64)
        tenant[lst[list(pos)]] = 1
        tenant[short[[0, 9]]] = 1                       # ... and the first and last position of the short list
        f = Filtered(pqv, st.s, st.n, doc, tenant)
        try:
            for kind, spec in ((EQ, [1] * 5), (RANGE, ([1] * 5, [5] * 5)), (IN, [[1, 9]] * 5)):
                for k, m in ((1, None), (10, None), (100, None), (5, 3)):
                    exp = f.check(st.queries, kind, spec, k, m, st.kc, f"positions {list(pos)[:4]}")
            assert exp[-2].max() > 0
        finally:
            f.close()


def test_nulls_on_different_rows_and_a_shared_mask(pqv, shape):
    """Case 3: NULL filter keys and NULL group keys on different rows, a shared mask ANDed in; the same RowKeys object as both columns."""
    st = shape
    tenant, doc = cases.columns(st.name, st.n, np.int32, np.int64)
    fvalid = (st.rng.random(st.n) >= 0.3).astype(np.uint8)
    gvalid = (st.rng.random(st.n) >= 0.3).astype(np.uint8)
    shared = st.rng.random(st.n) < 0.5
    f = Filtered(pqv, st.s, st.n, doc, tenant, gvalid, fvalid, shared)
    try:
        for kind in cases.KINDS:
            for k, m in ((5, None), (65, None), (13, 5)):
                exp = f.check(st.queries, cases.KINDS[kind], cases.SPECS[kind], k, m, 3, metric=st.metric)
                found = exp[0][exp[0] != EMPTY].astype(np.int64)
                assert len(found) and fvalid[found].all() and gvalid[found].all() and shared[found].all()
    finally:
        f.close()
    # group_keys and filter_keys the same object: "the nearest docs among the docs 0 .. 39", a doc IN-list
    f = Filtered(pqv, st.s, st.n, doc, doc, gvalid, gvalid)
    try:
        assert f.fkeys is f.gkeys
        for kind, spec in ((RANGE, ([0, 5, 0, 30, 9], [39, 5, 200, 10, 9])), (IN, [list(range(40)), [3], [1, 2], [], list(range(0, 90, 3))])):
            for k, m in ((5, None), (65, None), (13, 5)):
                f.check(st.queries, kind, spec, k, m, st.kc, "same column", metric=st.metric)
    finally:
        f.close()


def test_filters_that_match_nothing_or_lie_out_of_range(pqv, oracle):
    """Case 4: a key no row has, an empty IN slice, a RANGE with a > b: 0xFFFFFFFF / +inf / 0 everywhere.  An IN slice of 1024
    values.  Keys beyond the i32 range on an I32 column."""
    st = Setup(pqv, oracle, 4096, 128, 8, seed=23)
    tenant, doc = cases.columns("4096x128", st.n, np.int32, np.int32)
    f = Filtered(pqv, st.s, st.n, doc, tenant)
    nq = len(st.queries)
    try:
        for kind, spec in ((EQ, [99] * nq), (IN, [[]] * nq), (RANGE, ([5] * nq, [4] * nq)), (EQ, [2 ** 32 + 3] * nq),
                           (RANGE, ([2 ** 31] * nq, [I64_MAX] * nq)), (IN, [[2 ** 32, 2 ** 32 + 3, -(2 ** 32) + 3]] * nq)):
            for k, m in ((5, None), (65, None), (13, 5)):
                for form in (f.host, f.device):
                    got = form(st.queries, kind, spec, k, m, 3)
                    assert (got[0] == EMPTY).all() and np.isposinf(got[1]).all() and (got[2] == 0).all() and (got[-2] == 0).all()
                    assert (got[-1] == st.s.topk(st.queries, 1, 3)[3]).all()
                    if m is not None:
                        assert (got[3] == 0).all()
                f.check(st.queries, kind, spec, k, m, 3, "nothing")
        # 1024 values: every even value of [-1024, 1024) -- the tenants 0, 2, 4, 6 -- and ranges that reach beyond i32 on both sides
        big = list(range(-1024, 1024, 2))
        assert len(big) == 1024
        for kind, spec in ((IN, [big, big[:1023], [7] + big[:1000], big, [1]]),
                           (RANGE, ([-(2 ** 40), I64_MIN, 3, 2 ** 31 - 1, -1], [2, I64_MAX, 2 ** 40, 2 ** 33, 0]))):
            for k, m in ((5, None), (200, None), (33, 8)):
                exp = f.check(st.queries, kind, spec, k, m, st.kc, "wide filter values")
            assert (exp[-2][:3] > 0).all()
    finally:
        f.close()


@pytest.mark.parametrize("name", ["4096x128", "1500x30"])
def test_max_candidates_cuts_before_the_filter(pqv, oracle, name):
    """Case 5: the cap falls inside the second probed list, and inside the first; n_candidates stays the uncapped count."""
    c = SHAPES[name]
    st = Setup(pqv, oracle, c["n"], c["dim"], c["kc"], seed=21)
    tenant, doc = cases.columns(name, st.n, np.int64, np.int32)
    f = Filtered(pqv, st.s, st.n, doc, tenant)
    try:
        first = min(len(st.lists[int(st.oidx.find_closest_centroids(q, 1)[0])]) for q in st.queries)
        for cap in (first + 100, 37):
            for kind in cases.KINDS:
                kd, spec = cases.KINDS[kind], cases.SPECS[kind]
                exp = f.check(st.queries, kd, spec, 13, None, 3, f"cap={cap}", max_candidates=cap)
                f.check(st.queries, kd, spec, 13, 5, 3, f"cap={cap}", max_candidates=cap)
                q = st.queries[0]
                r, d2, g, nc, _ = ref.distinct_topk(st.oidx.candidate_rows(q, 3), doc, None, tenant, None, kd, spec, 0, None, st.data, q, 13,
                                                    max_candidates=cap)
                n = int(exp[3][0])
                assert n == len(r) and (exp[0][0, :n] == r).all() and (_bits(exp[1][0, :n]) == _bits(d2)).all() and exp[4][0] == nc
    finally:
        f.close()


def test_integer_data_ties_follow_d2_then_position(pqv, oracle):
    """Case 6: whole distance classes tie: representatives, ranks and a group's rows follow (d2, position)."""
    st = Setup(pqv, oracle, 3000, 8, 6, seed=4, integer=True)
    q = np.random.default_rng(2).integers(0, 3, (5, 8)).astype(np.float32)
    rng = np.random.default_rng(5)
    tenant, doc = rng.integers(0, 4, st.n).astype(np.int32), rng.integers(0, st.n // 16, st.n).astype(np.int64)
    f = Filtered(pqv, st.s, st.n, doc, tenant)
    try:
        for kind, spec in ((EQ, [0, 1, 2, 3, 1]), (RANGE, ([0, 1, 2, 0, 3], [1, 3, 2, 3, 0])), (IN, [[0, 2], [1], [0, 1, 2, 3], [3, 7], []])):
            for (k, m), nprobe in (((5, None), 2), ((65, None), st.kc), ((33, 8), st.kc), ((5, 3), 2)):
                exp = f.check(q, kind, spec, k, m, nprobe, "integer data")
            assert len(np.unique(_bits(exp[1][0]))) < exp[1][0].size          # (d2 is an integer <= 32: entries must tie)
        r, d2, g, _, _ = ref.distinct_topk(st.oidx.candidate_rows(q[0], 2), doc, None, tenant, None, EQ, [0], 0, None, st.data, q[0], 65)
        got = f.host(q[:1], EQ, [0], 65, None, 2)
        n = int(got[3][0])
        assert n == len(r) and (got[0][0, :n] == r).all() and (_bits(got[1][0, :n]) == _bits(d2)).all() and (got[2][0, :n] == g).all()
    finally:
        f.close()


def test_grouped(pqv, shape):
    """Case 7: group_size 2, 3, 8 with k * m <= 1024, (33, 8) among them; group_rows; group_size == 1 is the filtered distinct
    call; the embeddings_fetched delta is the considered rows plus pass 2's rows."""
    st = shape
    tenant, doc = cases.columns(st.name, st.n, np.int32, np.int64)
    f = Filtered(pqv, st.s, st.n, doc, tenant)
    try:
        for kind in cases.KINDS:
            kd, spec = cases.KINDS[kind], cases.SPECS[kind]
            for (k, m), nprobe in (((1, 2), 1), ((5, 3), 3), ((33, 8), st.kc), ((128, 8), 3), ((64, 4), st.kc)):
                exp = f.check(st.queries, kd, spec, k, m, nprobe, metric=st.metric)
            assert exp[3].max() > 1                      # (groups of several rows were returned)
            # m = 1: the filtered distinct call, padding included, and group_rows = 1 per found group
            for form in (f.host, f.device):
                d1, g1 = form(st.queries, kd, spec, 65, None, 3, metric=st.metric), form(st.queries, kd, spec, 65, 1, 3, metric=st.metric)
                assert (g1[0][:, :, 0] == d1[0]).all() and (_bits(g1[1][:, :, 0]) == _bits(d1[1])).all() and (g1[2] == d1[2]).all()
                assert (g1[4] == d1[3]).all() and (g1[5] == d1[4]).all() and (g1[3] == (np.arange(65)[None, :] < d1[3][:, None])).all()
        # the second opinion and the counters
        kd, spec = EQ, cases.SPECS["eq"]
        k, m, nprobe = 10, 3, 3
        cons = second = tot = 0
        for qi, q in enumerate(st.queries):
            cand = st.oidx.candidate_rows(q, nprobe)
            r, d2, g, c, nf, nc, ncons = ref.grouped_topk(cand, doc, None, tenant, None, kd, spec, qi, None, st.data, q, k, m, metric=st.metric)
            got = f.host(st.queries, kd, spec, k, m, nprobe, metric=st.metric)
            assert int(got[4][qi]) == nf and (got[0][qi] == r).all() and (_bits(got[1][qi]) == _bits(d2)).all()
            assert (got[2][qi] == g).all() and (got[3][qi] == c).all() and got[5][qi] == nc
            allow = f.allowed(kd, spec, qi)
            rows = cand[allow[cand.astype(np.int64)]].astype(np.int64)
            cons += len(rows); tot += len(cand)
            second += int(np.isin(doc[rows], g[:nf]).sum())
        assert 0 < second < cons
        for call in (f.host, f.device):
            before = st.s.counters()
            call(st.queries, kd, spec, k, m, nprobe, metric=st.metric)
            after = st.s.counters()
            assert after["embeddings_fetched"] - before["embeddings_fetched"] == cons + second
            assert after["candidate_rows"] - before["candidate_rows"] == tot
            assert after["queries"] - before["queries"] == len(st.queries)
    finally:
        f.close()


def test_cosine_row_order_and_a_three_file_table(pqv, oracle):
    """Case 8: PQV_COSINE, PQV_LAYOUT_ROW_ORDER, and a three-file table searcher with a gap between the row ranges."""
    from test_gpu_table import Table
    st = Setup(pqv, oracle, 2048, 256, 4, seed=33)
    tenant, doc = cases.columns("2048x256", st.n, np.int32, np.int32)
    f = Filtered(pqv, st.s, st.n, doc, tenant, None, (st.rng.random(st.n) >= 0.2).astype(np.uint8))
    try:
        for kind in cases.KINDS:
            for k, m in ((5, None), (65, None), (33, 8)):
                f.check(st.queries, cases.KINDS[kind], cases.SPECS[kind], k, m, 2, "cosine", metric=pqv.PQV_COSINE)
    finally:
        f.close()
    st = Setup(pqv, oracle, 1500, 132, 6, seed=14, flags=pqv.PQV_LAYOUT_ROW_ORDER)
    tenant, doc = cases.columns("1500x30", st.n, np.int64, np.int64)
    f = Filtered(pqv, st.s, st.n, doc, tenant)
    try:
        for kind in cases.KINDS:
            for k, m in ((5, None), (65, None), (13, 5)):
                f.check(st.queries, cases.KINDS[kind], cases.SPECS[kind], k, m, 3, "row order")
    finally:
        f.close()
    rng = np.random.default_rng(12)
    t = Table(pqv, oracle, rng, [900, 1400, 600], [4, 6, 3], 32, gap=5)
    n = len(t.data)
    tenant, doc = rng.integers(0, 8, n).astype(np.int32), rng.integers(0, n // 16, n).astype(np.int64)
    f = Filtered(pqv, t.s, n, doc, tenant, None, None, rng.random(n) < 0.7)
    queries = rng.random((5, 32), dtype=np.float32)
    try:
        for kind in cases.KINDS:
            kd, spec = cases.KINDS[kind], cases.SPECS[kind]
            for nprobe in (1, 2):
                f.check(queries, kd, spec, 5, None, nprobe, "table")
                f.check(queries, kd, spec, 13, 5, nprobe, "table")
            q = queries[0]
            r, d2, g, nc, _ = ref.distinct_topk(t.cand(q, 2), doc, None, tenant, None, kd, spec, 0, f.shared, t.data, q, 5)
            got = f.host(queries, kd, spec, 5, None, 2)
            n0 = int(got[3][0])
            assert n0 == len(r) and (got[0][0, :n0] == r).all() and (_bits(got[1][0, :n0]) == _bits(d2)).all() and got[4][0] == nc
    finally:
        f.close()


def test_equivalences(pqv, shape):
    """Case 9: the full-range filter on a column without NULLs is pqv_topk_distinct / pqv_topk_grouped bit for bit; with all group
    keys distinct, slot 0 holds topk_device(keys=, ...)'s result."""
    import torch
    from test_gpu_distinct import _device as distinct_device
    from test_gpu_grouped import _device as grouped_device
    st = shape
    tenant, doc = cases.columns(st.name, st.n, np.int32, np.int64)
    nq = len(st.queries)
    f = Filtered(pqv, st.s, st.n, doc, tenant, (st.rng.random(st.n) >= 0.3).astype(np.uint8))
    full = ([I64_MIN] * nq, [I64_MAX] * nq)
    try:
        for k, nprobe in ((1, 1), (65, 3), (200, st.kc)):
            for exp, got in ((st.s.topk_distinct(st.queries, k, nprobe, f.gkeys, metric=st.metric, sqrt_out=False),
                              f.host(st.queries, RANGE, full, k, None, nprobe, metric=st.metric)),
                             (distinct_device(st.s, st.queries, k, nprobe, f.gkeys, metric=st.metric),
                              f.device(st.queries, RANGE, full, k, None, nprobe, metric=st.metric))):
                for x, y in zip(got, exp):
                    assert x.tobytes() == np.asarray(y).astype(x.dtype).tobytes(), f"full range, distinct k={k}"
        for exp, got in ((st.s.topk_grouped(st.queries, 33, 8, 3, f.gkeys, metric=st.metric, sqrt_out=False),
                          f.host(st.queries, RANGE, full, 33, 8, 3, metric=st.metric)),
                         (grouped_device(st.s, st.queries, 33, 8, 3, f.gkeys, metric=st.metric),
                          f.device(st.queries, RANGE, full, 33, 8, 3, metric=st.metric))):
            for x, y in zip(got, exp):
                assert x.tobytes() == np.asarray(y).astype(x.dtype).tobytes(), "full range, grouped"
    finally:
        f.close()
    f = Filtered(pqv, st.s, st.n, st.rng.permutation(st.n).astype(np.int64) - st.n // 2, tenant)
    dev = torch.device("cuda", 0)
    q_t = torch.from_numpy(st.queries).to(dev)
    try:
        for kind in cases.KINDS:
            kd, spec = cases.KINDS[kind], cases.SPECS[kind]
            fkw, alive = _filter_tensors(kd, spec, dev)
            for (k, m), nprobe in (((64, None), 3), ((64, 4), 3), ((200, None), st.kc)):
                r_t = torch.full((nq, k), -1, dtype=torch.int32, device=dev); d_t = torch.zeros((nq, k), dtype=torch.float32, device=dev)
                nf_t = torch.zeros(nq, dtype=torch.int32, device=dev); nc_t = torch.zeros(nq, dtype=torch.int64, device=dev)
                st.s.topk_device(q_t.data_ptr(), nq, k, nprobe, r_t.data_ptr(), d_t.data_ptr(), nf_t.data_ptr(), nc_t.data_ptr(), sqrt_out=False,
                                 metric=st.metric, keys=f.fkeys, **fkw)
                torch.cuda.synchronize()
                rows, dist = r_t.cpu().numpy().view(np.uint32), d_t.cpu().numpy()
                for got in (f.host(st.queries, kd, spec, k, m, nprobe, metric=st.metric), f.device(st.queries, kd, spec, k, m, nprobe, metric=st.metric)):
                    g_r, g_d = (got[0], got[1]) if m is None else (got[0][:, :, 0], got[1][:, :, 0])
                    assert (g_r == rows).all() and (_bits(g_d) == _bits(dist)).all(), f"all keys distinct kind={kind} k={k} m={m}"
                    assert (got[-2] == nf_t.cpu().numpy()).all() and (got[-1] == nc_t.cpu().numpy()).all()
            del alive
    finally:
        f.close()


def test_beyond_the_kernel_lists_and_dot(pqv, oracle):
    """Case 10: k = 1100 and 1100 probed lists: the host forms fall back (the filtered range machinery and a host pass), the device
    forms return the twins' UNSUPPORTED texts; PQV_DOT is refused with the existing text."""
    device_text = "the device entry points take k <= 1024 and min\\(nprobe, n_clusters\\) <= 1024"
    grouped_text = "pqv_topk_grouped_device takes k \\* group_size <= 1024 and at most 1024 probed lists per query"
    st = Setup(pqv, oracle, 4096, 128, 8, seed=35)
    tenant = st.rng.integers(0, 2, st.n).astype(np.int32)
    doc = st.rng.integers(0, st.n, st.n).astype(np.int64)               # (about 1200 docs among a tenant's considered rows)
    f = Filtered(pqv, st.s, st.n, doc, tenant, None, (st.rng.random(st.n) >= 0.2).astype(np.uint8), st.rng.random(st.n) < 0.9)
    q = st.queries[:2]
    try:
        for kind, spec in ((EQ, [1, 0]), (RANGE, ([0, 1], [1, 1])), (IN, [[0], [0, 1]])):
            exp = f.check(q, kind, spec, 1100, None, st.kc, forms=("host",))
            assert exp[3].max() == 1100
            exp = f.check(q, kind, spec, 205, 5, st.kc, forms=("host",))
            assert (exp[4] == 205).all()
            with pytest.raises(pqv.PqvError, match=device_text) as e:
                f.device(q, kind, spec, 1100, None, st.kc)
            assert e.value.code == -5
            with pytest.raises(pqv.PqvError, match=grouped_text) as e:
                f.device(q, kind, spec, 205, 5, st.kc)
            assert e.value.code == -5
            for form in (f.host, f.device):
                for m in (None, 3):
                    with pytest.raises(pqv.PqvError, match="PQV_DOT is not supported by keyed and distinct calls") as e:
                        form(q, kind, spec, 5, m, 2, metric=pqv.PQV_DOT)
                    assert e.value.code == -5
    finally:
        f.close()
    st = Setup(pqv, oracle, 2200, 8, 1100, seed=15)
    tenant, doc = st.rng.integers(0, 4, st.n).astype(np.int64), st.rng.integers(0, st.n // 16, st.n).astype(np.int32)
    f = Filtered(pqv, st.s, st.n, doc, tenant)
    q = st.queries[:2]
    try:
        for kind, spec in ((EQ, [1, 3]), (IN, [[0, 2], [1]])):
            exp = f.check(q, kind, spec, 10, None, 1100, forms=("host",))
            f.check(q, kind, spec, 10, 3, 1100, forms=("host",))
            assert (exp[3] == 10).all()
            r, d2, g, nc, _ = ref.distinct_topk(st.oidx.candidate_rows(q[0], 1100), doc, None, tenant, None, kind, spec, 0, None, st.data, q[0], 10)
            assert (exp[0][0] == r).all() and (_bits(exp[1][0]) == _bits(d2)).all() and (exp[2][0] == g).all() and exp[4][0] == nc
            with pytest.raises(pqv.PqvError, match=device_text):
                f.device(q, kind, spec, 10, None, 1100)
            with pytest.raises(pqv.PqvError, match=grouped_text):
                f.device(q, kind, spec, 10, 3, 1100)
    finally:
        f.close()


@pytest.mark.parametrize("name,kind", [("132", "eq"), ("134", "range"), ("768", "in"), ("70-seq", "range"), ("132-cos", "in")])
def test_multi_chunk_rows(pqv, oracle, name, kind):
    """Case 11: the chunk loop runs more than once (long_rows_cases.SHAPES), with that module's Case inputs -- its tenant column
    (NULLs included) as the filter column, its group column, its per-query filters -- against both the yardstick and the Case's
    CPU reference under M_q."""
    import long_rows_cases as L
    from test_gpu_long_rows import Live
    live = Live(pqv, oracle, name)
    case = live.case
    wide = name in ("134", "768")
    tenant = L.wide(case.tenant) if wide else case.tenant
    w = (lambda v: [int(x) for x in L.wide(v)]) if wide else (lambda v: list(v))
    kd = cases.KINDS[kind]
    spec = {"eq": w(L.QUERY_KEYS), "range": (w(L.QUERY_RANGES[0]), w(L.QUERY_RANGES[1])), "in": [w(s) for s in L.QUERY_SETS]}[kind]
    f = Filtered(pqv, live.s, case.n, case.group, tenant, case.group_valid, case.tenant_valid, case.masks["1/2"])
    try:
        for nprobe in L.NPROBES:
            for k, m in ((10, None), (100, None), (5, 3), (33, 8)):
                got = f.check(live.q, kd, spec, k, m, nprobe, name, metric=live.metric)
                for qi in range(L.NQ):
                    mq = f.allowed(kd, spec, qi)
                    if m is None:
                        r, d, g, c, _ = ref.distinct_ref.distinct_topk(case.cand(qi, nprobe), case.group, case.group_valid, mq, case.rdata,
                                                                       case.rq[qi], k, metric=case.metric)
                        n = len(r)
                        assert int(got[3][qi]) == n and (got[0][qi, :n] == r).all() and (got[2][qi, :n] == g).all() and got[4][qi] == c
                        assert (_bits(got[1][qi, :n]) == _bits(case._out(d, False))).all()
                    else:
                        r, d, g, cnt, nf, c, _ = ref.grouped_ref.grouped_topk(case.cand(qi, nprobe), case.group, case.group_valid, mq, case.rdata,
                                                                             case.rq[qi], k, m, metric=case.metric)
                        assert int(got[4][qi]) == nf and (got[0][qi] == r).all() and (got[2][qi] == g).all() and (got[3][qi] == cnt).all()
                        fin = np.isfinite(d)
                        assert (_bits(got[1][qi][fin]) == _bits(case._out(d[fin], False))).all() and got[5][qi] == c
    finally:
        f.close()


def test_device_form_is_asynchronous_with_device_resident_filters(pqv, oracle):
    """Case 12: the device forms read the filter arrays on the stream inside the enqueued work: the arrays are written by a copy
    enqueued on the SAME stream just before the call, the outputs are pre-filled with garbage, and there is one synchronise behind
    everything; a second submission through the same lane is bit-equal; the optional outputs may be NULL."""
    import torch
    st = Setup(pqv, oracle, 4096, 128, 8, seed=19)
    tenant, doc = cases.columns("4096x128", st.n, np.int32, np.int64)
    f = Filtered(pqv, st.s, st.n, doc, tenant)
    dev = torch.device("cuda", 0)
    nq, k, m = len(st.queries), 13, 5
    stream = torch.cuda.Stream(device=dev)
    try:
        for kind in cases.KINDS:
            kd, spec = cases.KINDS[kind], cases.SPECS[kind]
            _, a, b = ref.descriptor(kd, spec)
            h_a = torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).pin_memory()
            h_b = torch.from_numpy(np.ascontiguousarray(b if b is not None and len(b) else np.zeros(1, np.int64))).pin_memory()
            h_q = torch.from_numpy(st.queries).pin_memory()
            outs = []
            with torch.cuda.stream(stream):
                d_a = torch.full(h_a.shape, -7, dtype=torch.int64, device=dev); d_b = torch.full(h_b.shape, -7, dtype=torch.int64, device=dev)
                q_t = torch.zeros(st.queries.shape, dtype=torch.float32, device=dev)
                fkw = ({"query_keys": d_a.data_ptr()} if kd == EQ else
                       {("query_key_ranges" if kd == RANGE else "query_key_sets"): (d_a.data_ptr(), d_b.data_ptr())})
                for rep in range(2):
                    r1 = torch.full((nq, k), 5, dtype=torch.int32, device=dev); d1 = torch.full((nq, k), -1.0, dtype=torch.float32, device=dev)
                    g1 = torch.full((nq, k), 77, dtype=torch.int64, device=dev); n1 = torch.full((nq,), 9, dtype=torch.int32, device=dev)
                    r2 = torch.full((nq, k, m), 5, dtype=torch.int32, device=dev); d2 = torch.full((nq, k, m), -1.0, dtype=torch.float32, device=dev)
                    c2 = torch.full((nq, k), 99, dtype=torch.int32, device=dev)
                    # the inputs arrive on the stream, the calls are enqueued behind them, nothing waits in between
                    q_t.copy_(h_q, non_blocking=True); d_a.copy_(h_a, non_blocking=True); d_b.copy_(h_b, non_blocking=True)
                    st.s.topk_distinct_device(q_t.data_ptr(), nq, k, 3, f.gkeys, r1.data_ptr(), d1.data_ptr(), g1.data_ptr(), n1.data_ptr(),
                                              sqrt_out=False, stream=stream.cuda_stream, filter_keys=f.fkeys, **fkw)
                    st.s.topk_grouped_device(q_t.data_ptr(), nq, k, m, 3, f.gkeys, r2.data_ptr(), d2.data_ptr(), 0, c2.data_ptr(),
                                             sqrt_out=False, stream=stream.cuda_stream, filter_keys=f.fkeys, **fkw)
                    outs.append((r1, d1, g1, n1, r2, d2, c2))
            stream.synchronize()
            exp_d = f.yardstick(st.queries, kd, spec, k, None, 3)
            exp_g = f.yardstick(st.queries, kd, spec, k, m, 3)
            for r1, d1, g1, n1, r2, d2, c2 in outs:
                assert (r1.cpu().numpy().view(np.uint32) == exp_d[0]).all() and (_bits(d1.cpu().numpy()) == _bits(exp_d[1])).all()
                assert (g1.cpu().numpy() == exp_d[2]).all() and (n1.cpu().numpy() == exp_d[3]).all()
                assert (r2.cpu().numpy().view(np.uint32) == exp_g[0]).all() and (_bits(d2.cpu().numpy()) == _bits(exp_g[1])).all()
                assert (c2.cpu().numpy().view(np.uint32) == exp_g[3]).all()
        # sqrt_out: the IEEE square root of the same d2
        kd, spec = EQ, cases.SPECS["eq"]
        a, b = f.host(st.queries, kd, spec, k, None, 3, sqrt_out=True), f.host(st.queries, kd, spec, k, None, 3)
        assert (a[0] == b[0]).all() and (_bits(a[1]) == _bits(np.sqrt(b[1]))).all()
    finally:
        f.close()
