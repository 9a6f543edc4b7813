"""Per-query key filters on the GPU (pqv_row_keys, pqv_topk_keyed / pqv_topk_keyed_device / pqv_range_search_keyed).

The yardstick everywhere is the EXISTING masked path: the queries of a keyed call are grouped by key and each distinct key is
one searcher.row_mask(M_key) call over its queries, M_key = tests/keyed_ref.py's allowed_for(column, valid, key, shared mask).
Rows, distance bits, n_found / n_within, n_candidates, tie flags and lims must be equal.  Capped calls and the paths beyond the
kernels' lists are held to tests/mask_ref.py as well."""
import numpy as np
import pytest

import keyed_ref
import mask_ref
from pq_vector_amd import _ffi
from test_gpu_mask import SHAPES, Setup, _bits, _same

pytestmark = pytest.mark.gpu

EMPTY = 0xFFFFFFFF
NQ = 7


def _device(s, q, k, nprobe, flags, mask=None, keys=None, qkeys=None, metric=0, max_candidates=0):
    """topk_device with d2 output -> (rows, dist, n_found, n_candidates, tie flags or None)"""
    import torch
    dev = torch.device("cuda", 0)
    q_t = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(dev)
    nq = len(q)
    r_t = torch.full((nq, k), -1, dtype=torch.int32, device=dev)
    d_t = torch.full((nq, k), float("inf"), dtype=torch.float32, device=dev)
    nf_t = torch.zeros(nq, dtype=torch.int32, device=dev)
    nc_t = torch.zeros(nq, dtype=torch.int64, device=dev)
    tf_t = torch.full((nq,), 7, dtype=torch.int32, device=dev)
    kw = {}
    if mask is not None:
        kw["mask"] = mask
    if keys is not None:
        qk_t = torch.from_numpy(np.ascontiguousarray(qkeys, dtype=np.int64)).to(dev)
        kw.update(keys=keys, query_keys=qk_t.data_ptr())
    torch.cuda.synchronize()
    s.topk_device(q_t.data_ptr(), nq, k, nprobe, r_t.data_ptr(), d_t.data_ptr(), nf_t.data_ptr(), nc_t.data_ptr(), sqrt_out=False,
                  max_candidates=max_candidates, metric=metric, d_tie_flags=tf_t.data_ptr() if flags else 0, **kw)
    torch.cuda.synchronize()
    return (r_t.cpu().numpy().view(np.uint32), d_t.cpu().numpy(), nf_t.cpu().numpy().astype(np.uint32),
            nc_t.cpu().numpy().astype(np.uint64), tf_t.cpu().numpy() if flags else None)


def _split_range(res, nq):
    """range_search's (lims, rows, dist, n_within, n_candidates) -> per query (rows, dist bits, n_within, n_candidates)"""
    lims, rows, dist, nw, nc = res
    assert len(lims) == nq + 1 and lims[0] == 0 and lims[-1] == len(rows) == len(dist)
    return [(rows[int(lims[i]):int(lims[i + 1])], _bits(dist[int(lims[i]):int(lims[i + 1])]), int(nw[i]), int(nc[i])) for i in range(nq)]


def _same_range(got, exp, what):
    assert len(got) == len(exp)
    for i, (g, e) in enumerate(zip(got, exp)):
        assert len(g[0]) == len(e[0]) and (g[0] == e[0]).all() and (g[1] == e[1]).all() and g[2:] == e[2:], f"{what}: query {i} differs"


class Keyed:
    """A key column over a searcher's rows, its RowKeys, and the yardstick: one masked call per distinct key."""

    def __init__(self, pqv, s, n, values, valid=None, shared=None):
        self.pqv, self.s, self.values, self.valid, self.shared = pqv, s, values, valid, shared
        self.column = pqv.Column.upload(values, valid, device=0)
        self.keys = s.row_keys(self.column)
        assert self.keys.rows == n and self.keys.dtype == (_ffi.PQV_COL_I32 if values.dtype == np.int32 else _ffi.PQV_COL_I64)
        self.column.close()                  # (the keys copied what they need: the column is gone before the first search)
        self.shared_mask = s.row_mask(shared) if shared is not None else None
        self._masks = {}

    def allowed(self, key):
        return keyed_ref.allowed_for(self.values, self.valid, key, self.shared)

    def mask(self, key):
        if key not in self._masks:
            self._masks[key] = self.s.row_mask(self.allowed(key))
        return self._masks[key]

    def close(self):
        for m in self._masks.values():
            m.close()
        if self.shared_mask is not None:
            self.shared_mask.close()
        self.keys.close()

    # --- the keyed calls
    def topk(self, q, qkeys, k, nprobe, **kw):
        return self.s.topk(q, k, nprobe, keys=self.keys, query_keys=qkeys, mask=self.shared_mask, **kw)

    def device(self, q, qkeys, k, nprobe, flags, **kw):
        return _device(self.s, q, k, nprobe, flags, mask=self.shared_mask, keys=self.keys, qkeys=qkeys, **kw)

    def range(self, q, qkeys, radius, nprobe, **kw):
        return _split_range(self.s.range_search(q, radius, nprobe, keys=self.keys, query_keys=qkeys, mask=self.shared_mask, **kw), len(q))

    # --- the yardstick: the same queries grouped by key, one masked call per distinct key
    def _grouped(self, q, qkeys, call):
        out = [None] * len(q)
        for key, idx in keyed_ref.group_by_key(qkeys).items():
            res = call(q[idx], self.mask(key))
            for j, i in enumerate(idx):
                out[i] = res[j]
        return out

    def y_topk(self, q, qkeys, k, nprobe, **kw):
        per = self._grouped(q, qkeys, lambda qq, m: list(zip(*self.s.topk(qq, k, nprobe, mask=m, **kw))))
        return tuple(np.stack([p[c] for p in per]) for c in range(4))

    def y_device(self, q, qkeys, k, nprobe, flags, **kw):
        n_out = 5 if flags else 4
        per = self._grouped(q, qkeys, lambda qq, m: list(zip(*_device(self.s, qq, k, nprobe, flags, mask=m, **kw)[:n_out])))
        return tuple(np.stack([p[c] for p in per]) for c in range(n_out)) + (() if flags else (None,))

    def y_range(self, q, qkeys, radius, nprobe, **kw):
        return self._grouped(q, qkeys, lambda qq, m: _split_range(self.s.range_search(qq, radius, nprobe, mask=m, **kw), len(qq)))


def _tenant_ids(t, dtype):
    """t distinct keys with negatives among them; int64: most are beyond +-2^32"""
    base = np.arange(t, dtype=np.int64) - t // 3
    return (base * 1009).astype(np.int32) if dtype == np.int32 else base * (2 ** 32 + 12345)


def _column(rng, n, tenants, dtype, nulls):
    """-> (values [n], valid or None, ids): tenants = 0 gives every row its own key"""
    ids = _tenant_ids(tenants if tenants else n, dtype)
    values = (ids[rng.integers(0, tenants, n)] if tenants else ids[rng.permutation(n)]).astype(dtype)
    valid = (rng.random(n) >= 1 / 8).astype(np.uint8) if nulls else None
    return values, valid, ids


def _query_keys(rng, values, ids):
    """7 keys: two queries share one, one is absent from the column, one is 2^32 + a present value (matches nothing on an int32
    column; on an int64 column it is an ordinary -- most likely absent -- key), the rest are present"""
    present = values[rng.integers(0, len(values), 5)].astype(np.int64)
    absent = int(ids.astype(np.int64).max()) + 1
    qk = [int(present[0]), int(present[1]), int(present[0]), absent, int(present[2]), 2 ** 32 + int(present[3]), int(present[4])]
    assert not (values.astype(np.int64) == absent).any()
    if values.dtype == np.int32:
        assert not (values.astype(np.int64) == qk[5]).any() and (values == np.int64(qk[5]).astype(np.int32)).any()   # (truncation WOULD match)
    return np.array(qk, np.int64)


@pytest.fixture(scope="module", params=list(SHAPES))
def shape(request, pqv, oracle):
    c = SHAPES[request.param]
    st = Setup(pqv, oracle, c["n"], c["dim"], c["kc"], seed=11 + c["dim"])
    st.metric = c["metric"]
    st.q7 = np.random.default_rng(5 + c["dim"]).random((NQ, c["dim"]), dtype=np.float32)
    return st


def _check_all_entry_points(st, kd, q, qkeys, ks, nprobes, metric, what):
    nc_unfiltered = st.s.topk(q, 1, max(nprobes), metric=metric)[3] if nprobes else None
    for nprobe in nprobes:
        for k in ks:
            w = f"{what} k={k} nprobe={nprobe}"
            got, exp = kd.topk(q, qkeys, k, nprobe, metric=metric), kd.y_topk(q, qkeys, k, nprobe, metric=metric)
            _same(got, exp, "topk " + w)
            assert (got[2] <= k).all()
            for flags in (False, True):
                got = kd.device(q, qkeys, k, nprobe, flags, metric=metric)
                exp = kd.y_device(q, qkeys, k, nprobe, flags, metric=metric)
                _same(got[:4], exp[:4], f"device flags={flags} " + w)
                if flags:
                    assert (got[4] == exp[4]).all(), "tie flags " + w
        r = st.radius(nprobe, metric)
        for max_results in (0, 7):
            _same_range(kd.range(q, qkeys, r, nprobe, max_results=max_results, metric=metric),
                        kd.y_range(q, qkeys, r, nprobe, max_results=max_results, metric=metric), f"range max_results={max_results} nprobe={nprobe} {what}")
    if nprobes:     # n_candidates stays the unfiltered count
        assert (kd.topk(q, qkeys, 1, max(nprobes), metric=metric)[3] == nc_unfiltered).all()


@pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
@pytest.mark.parametrize("dtype", [np.int32, np.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("tenants", [3, 64, 0], ids=["T3", "T64", "distinct"])
def test_keyed_calls_equal_one_masked_call_per_key(shape, tenants, dtype, nulls):
    """Case 1: k in {1, 10, 100, 300} (S = 1, 4, 16), nprobe in {1, 3, all}; topk, topk_device with and without tie flags,
    range_search with max_results in {0, 7}."""
    st = shape
    rng = np.random.default_rng(1000 * tenants + 10 * st.dim + 2 * nulls + (dtype == np.int64))
    values, valid, ids = _column(rng, st.n, tenants, dtype, nulls)
    qkeys = _query_keys(rng, values, ids)
    if not tenants:      # every key is one row: take the keys of rows the queries find, so that most queries have their one match
        near = st.s.topk(st.q7, 1, st.kc)[0][:, 0]
        for i in (0, 1, 4, 6):
            qkeys[i] = int(values[near[i]])
        qkeys[2] = qkeys[0]
    kd = Keyed(st.pqv, st.s, st.n, values, valid)
    try:
        _check_all_entry_points(st, kd, st.q7, qkeys, (1, 10, 100, 300), (1, 3, st.kc), st.metric, "")
        # the absent key and the out-of-range key on an int32 column: nothing, as the contract writes it
        rows, dist, nf, _ = kd.topk(st.q7, qkeys, 10, st.kc, metric=st.metric)
        empty = [3] + ([5] if dtype == np.int32 else [])
        for i in empty:
            assert nf[i] == 0 and (rows[i] == EMPTY).all() and np.isinf(dist[i]).all() and (dist[i] > 0).all()
        assert nf[0] == nf[2] and (rows[0][:nf[0]] != EMPTY).all()
        if tenants:
            assert nf[0] > 0
        hit = kd.range(st.q7, qkeys, 1e30, st.kc, metric=st.metric)
        for i in empty:
            assert len(hit[i][0]) == 0 and hit[i][2] == 0
    finally:
        kd.close()


@pytest.mark.parametrize("sel", [2, 64], ids=["1/2", "1/64"])
def test_keyed_with_a_shared_mask(shape, sel):
    """Case 2: keys AND one shared row mask == the masked call under M_key & mask."""
    st = shape
    rng = np.random.default_rng(77 + sel + st.dim)
    for tenants, dtype, nulls in ((3, np.int32, True), (64, np.int64, False)):
        values, valid, ids = _column(rng, st.n, tenants, dtype, nulls)
        qkeys = _query_keys(rng, values, ids)
        kd = Keyed(st.pqv, st.s, st.n, values, valid, shared=rng.random(st.n) < 1.0 / sel)
        try:
            _check_all_entry_points(st, kd, st.q7, qkeys, (10, 300), (3, st.kc), st.metric, f"shared 1/{sel}")
        finally:
            kd.close()


def test_ties_follow_the_reference_heap_under_keys(pqv, oracle):
    """Case 3: tie-heavy integer data, dim 8: the host form's heap replay and the device form's tie flags equal the yardstick's."""
    st = Setup(pqv, oracle, 3000, 8, 6, seed=4, integer=True)
    rng = np.random.default_rng(2)
    q = rng.integers(0, 3, (24, 8)).astype(np.float32)
    for tenants, dtype, nulls in ((3, np.int64, True), (64, np.int32, False)):
        values, valid, ids = _column(rng, st.n, tenants, dtype, nulls)
        qkeys = values[rng.integers(0, st.n, len(q))].astype(np.int64)
        qkeys[5] = int(ids.astype(np.int64).max()) + 1
        kd = Keyed(pqv, st.s, st.n, values, valid)
        before = st.s.counters()["exact_replays"]
        flagged = 0
        for k, nprobe in ((5, 2), (20, st.kc), (100, 3)):
            _same(kd.topk(q, qkeys, k, nprobe), kd.y_topk(q, qkeys, k, nprobe), f"tied host form k={k}")
            got, exp = kd.device(q, qkeys, k, nprobe, True), kd.y_device(q, qkeys, k, nprobe, True)
            _same(got[:4], exp[:4], f"tied device form k={k}")
            assert (got[4] == exp[4]).all()
            flagged += int(got[4].sum())
        assert flagged and st.s.counters()["exact_replays"] > before
        kd.close()


@pytest.mark.parametrize("name", ["4096x128", "1500x30", "2048x32-seq"])
def test_max_candidates_caps_before_the_keys(pqv, oracle, name):
    """Case 4, plain searcher: max_candidates in {1, 100, just below the total}: capped first, then filtered; the counters advance
    by the restatement's considered rows and the uncapped totals, summed over the batch."""
    c = SHAPES[name]
    st = Setup(pqv, oracle, c["n"], c["dim"], c["kc"], seed=21)
    metric = c["metric"]
    rng = np.random.default_rng(31)
    q = rng.random((NQ, c["dim"]), dtype=np.float32)
    values, valid, ids = _column(rng, st.n, 3, np.int32, True)
    qkeys = _query_keys(rng, values, ids)
    kd = Keyed(pqv, st.s, st.n, values, valid)
    cands = [st.oidx.candidate_rows(x, 3) for x in q]
    for cap in (1, 100, min(len(x) for x in cands) - 1):
        exp = [mask_ref.masked_topk(cands[i], kd.allowed(qkeys[i]), st.data, q[i], 10, metric=metric, max_candidates=cap) for i in range(NQ)]
        cons, tot = sum(e[3] for e in exp), sum(e[2] for e in exp)
        before = st.s.counters()
        got = kd.topk(q, qkeys, 10, 3, max_candidates=cap, metric=metric, sqrt_out=False)
        after = st.s.counters()
        assert after["embeddings_fetched"] - before["embeddings_fetched"] == cons
        assert after["candidate_rows"] - before["candidate_rows"] == tot
        assert after["queries"] - before["queries"] == NQ
        _same(got, kd.y_topk(q, qkeys, 10, 3, max_candidates=cap, metric=metric, sqrt_out=False), f"capped topk {cap}")
        before = st.s.counters()
        dv = kd.device(q, qkeys, 10, 3, True, max_candidates=cap, metric=metric)
        after = st.s.counters()
        assert after["embeddings_fetched"] - before["embeddings_fetched"] == cons
        assert after["candidate_rows"] - before["candidate_rows"] == tot
        _same(dv[:4], kd.y_device(q, qkeys, 10, 3, True, max_candidates=cap, metric=metric)[:4], f"capped device {cap}")
        for i, (rows, d2, nc, _) in enumerate(exp):
            n = int(got[2][i])
            assert n == len(rows) and (got[0][i, :n] == rows).all() and (_bits(got[1][i, :n]) == _bits(d2)).all() and got[3][i] == nc
            assert int(dv[2][i]) == n and (dv[0][i, :n] == rows).all() and (_bits(dv[1][i, :n]) == _bits(d2)).all()
        radius = 0.9 * float(np.sqrt(c["dim"] / 6.0))
        before = st.s.counters()
        rg = kd.range(q, qkeys, radius, 3, max_candidates=cap, metric=metric)
        after = st.s.counters()
        assert after["embeddings_fetched"] - before["embeddings_fetched"] == cons
        assert after["candidate_rows"] - before["candidate_rows"] == tot
        _same_range(rg, kd.y_range(q, qkeys, radius, 3, max_candidates=cap, metric=metric), f"capped range {cap}")
        for i in range(NQ):
            rr, rd, nw, nc = mask_ref.masked_range(cands[i], kd.allowed(qkeys[i]), st.data, q[i], radius, metric=metric, max_candidates=cap)
            assert (rg[i][0] == rr).all() and (rg[i][1] == _bits(rd)).all() and rg[i][2:] == (nw, nc)
    kd.close()


def test_table_round_robin_quotas_come_before_the_keys(pqv, oracle):
    """Case 4, table: three files under PQV_TABLE_CAP_ROUND_ROBIN, keys over CORPUS rows (the gaps between the files included)."""
    from test_gpu_table import Table
    from test_gpu_table_cap import _selected
    rng = np.random.default_rng(12)
    t = Table(pqv, oracle, rng, [900, 1400, 500], [4, 6, 3], 32, gap=5, flags=pqv.PQV_TABLE_CAP_ROUND_ROBIN)
    n = len(t.data)
    values, valid, ids = _column(rng, n, 3, np.int64, True)
    qkeys = _query_keys(rng, values, ids)
    q = rng.random((NQ, 32), dtype=np.float32)
    kd = Keyed(pqv, t.s, n, values, valid)
    for nprobe in (1, 2):
        for cap in (0, 500, 2000):
            sels = [_selected(t, oracle, x, nprobe, cap)[0] if cap else t.cand(x, nprobe) for x in q]
            exp = [mask_ref.masked_topk(sels[i], kd.allowed(qkeys[i]), t.data, q[i], 10) for i in range(NQ)]
            before = t.s.counters()
            got = kd.topk(q, qkeys, 10, nprobe, max_candidates=cap, sqrt_out=False)
            after = t.s.counters()
            assert after["embeddings_fetched"] - before["embeddings_fetched"] == sum(e[3] for e in exp)
            _same(got, kd.y_topk(q, qkeys, 10, nprobe, max_candidates=cap, sqrt_out=False), f"table topk cap={cap}")
            dv = kd.device(q, qkeys, 10, nprobe, True, max_candidates=cap)
            _same(dv[:4], kd.y_device(q, qkeys, 10, nprobe, True, max_candidates=cap)[:4], f"table device cap={cap}")
            for i, (rows, d2, _, _) in enumerate(exp):
                m = int(got[2][i])
                assert m == len(rows) and (got[0][i, :m] == rows).all() and (_bits(got[1][i, :m]) == _bits(d2)).all()
                assert got[3][i] == len(t.cand(q[i], nprobe))
            _same_range(kd.range(q, qkeys, 2.0, nprobe, max_candidates=cap), kd.y_range(q, qkeys, 2.0, nprobe, max_candidates=cap),
                        f"table range cap={cap}")
    kd.close()


def test_beyond_the_kernel_lists(pqv, oracle):
    """Case 5: k = 1500, and more than 1024 short lists at nprobe = all, through the host form; the device form is unsupported;
    range search with more than 1024 probed lists."""
    st = Setup(pqv, oracle, 2200, 8, 1100, seed=15)
    rng = np.random.default_rng(16)
    q = rng.random((NQ, 8), dtype=np.float32)
    values, valid, ids = _column(rng, st.n, 3, np.int32, True)
    qkeys = _query_keys(rng, values, ids)
    kd = Keyed(pqv, st.s, st.n, values, valid)
    for k, nprobe in ((10, 1100), (1500, 1100), (1500, 40)):
        before = st.s.counters()
        got = kd.topk(q, qkeys, k, nprobe, sqrt_out=False)
        after = st.s.counters()
        _same(got, kd.y_topk(q, qkeys, k, nprobe, sqrt_out=False), f"beyond: k={k} nprobe={nprobe}")
        cons = tot = 0
        for i in range(NQ):
            rows, d2, nc, ncons = mask_ref.masked_topk(st.oidx.candidate_rows(q[i], nprobe), kd.allowed(qkeys[i]), st.data, q[i], k)
            assert len(np.unique(_bits(d2))) == len(d2)
            n = int(got[2][i])
            assert n == len(rows) == min(k, ncons) and (got[0][i, :n] == rows).all() and (_bits(got[1][i, :n]) == _bits(d2)).all()
            assert got[3][i] == nc and (got[0][i, n:] == EMPTY).all()
            cons += ncons; tot += nc
        assert after["embeddings_fetched"] - before["embeddings_fetched"] == cons
        assert after["candidate_rows"] - before["candidate_rows"] == tot
        with pytest.raises(pqv.PqvError) as e:
            kd.device(q, qkeys, k, nprobe, False)
        assert e.value.code == -5
    rg = kd.range(q, qkeys, 0.5, 1100)
    _same_range(rg, kd.y_range(q, qkeys, 0.5, 1100), "range over 1100 probed lists")
    for i in range(NQ):
        rr, rd, nw, nc = mask_ref.masked_range(st.oidx.candidate_rows(q[i], 1100), kd.allowed(qkeys[i]), st.data, q[i], 0.5)
        assert (rg[i][0] == rr).all() and (rg[i][1] == _bits(rd)).all() and rg[i][2:] == (nw, nc)
    kd.close()


def test_keyed_cosine_equals_masked_cosine(pqv, oracle):
    """Case 6: metric = PQV_COSINE."""
    c = SHAPES["4096x128"]
    st = Setup(pqv, oracle, c["n"], c["dim"], c["kc"], seed=41)
    rng = np.random.default_rng(42)
    q = rng.random((NQ, c["dim"]), dtype=np.float32) - 0.5
    values, valid, ids = _column(rng, st.n, 64, np.int64, True)
    qkeys = _query_keys(rng, values, ids)
    kd = Keyed(pqv, st.s, st.n, values, valid)
    for k, nprobe in ((1, 1), (10, 3), (300, st.kc)):
        _same(kd.topk(q, qkeys, k, nprobe, metric=pqv.PQV_COSINE), kd.y_topk(q, qkeys, k, nprobe, metric=pqv.PQV_COSINE), f"cosine topk k={k}")
        got, exp = kd.device(q, qkeys, k, nprobe, True, metric=pqv.PQV_COSINE), kd.y_device(q, qkeys, k, nprobe, True, metric=pqv.PQV_COSINE)
        _same(got[:4], exp[:4], f"cosine device k={k}")
        assert (got[4] == exp[4]).all()
    radius = float(kd.topk(q, qkeys, 10, 3, metric=pqv.PQV_COSINE)[1][0, 5])
    assert np.isfinite(radius)
    _same_range(kd.range(q, qkeys, radius, 3, metric=pqv.PQV_COSINE), kd.y_range(q, qkeys, radius, 3, metric=pqv.PQV_COSINE), "cosine range")
    kd.close()


def test_host_sub_batches_slice_the_query_keys(pqv, oracle):
    """Case 7: one host call of more queries than one sub-batch of pqv_topk_impl holds (k = 300, 4096 x 128, all 8 lists: the
    plan's scratch per query against the 1 GiB bound, restated from the code) -- every query is right, so the keys were sliced
    with the queries."""
    c = SHAPES["4096x128"]
    st = Setup(pqv, oracle, c["n"], c["dim"], c["kc"], seed=51)
    k, nprobe, dim = 300, st.kc, c["dim"]
    k_int = k + 1
    n_part_rr = nprobe * 1 * 4              # exact stream, >= 8192 (query, list) pairs: one block of four waves per list
    n_part_probe, probe_kpart = 4, 64       # 8 centroids: one probe block of four waves; probe_rows_kernel's 64 unsorted entries
    per_query = n_part_rr * k_int * 12 + n_part_probe * probe_kpart * 12 + 8192 * 12 + nprobe * (dim + 32) + dim * 4 + 1
    batch = (1 << 30) // per_query
    nq = batch + batch // 2                 # (the second sub-batch starts in the middle of the call)
    assert 2000 < batch < 8000
    rng = np.random.default_rng(52)
    q = rng.random((nq, dim), dtype=np.float32)
    values, valid, ids = _column(rng, st.n, 64, np.int32, True)
    qkeys = values[rng.integers(0, st.n, nq)].astype(np.int64)
    kd = Keyed(pqv, st.s, st.n, values, valid)
    got = kd.topk(q, qkeys, k, nprobe)
    _same(got, kd.y_topk(q, qkeys, k, nprobe), "sub-batched host call")
    assert (got[2][batch:] > 0).all()
    r = st.radius(1)
    _same_range(kd.range(q[:200], qkeys[:200], r, 1), kd.y_range(q[:200], qkeys[:200], r, 1), "range")
    kd.close()


def test_query_keys_are_read_in_stream_order(pqv, oracle):
    """Case 8: d_qkeys is written by a torch op on a side stream and the keyed device call is enqueued on that stream with no
    synchronisation between."""
    import torch
    c = SHAPES["4096x128"]
    st = Setup(pqv, oracle, c["n"], c["dim"], c["kc"], seed=61)
    rng = np.random.default_rng(62)
    values, valid, ids = _column(rng, st.n, 64, np.int64, False)
    nq, k, nprobe = 64, 10, 3
    q = rng.random((nq, c["dim"]), dtype=np.float32)
    qkeys = values[rng.integers(0, st.n, nq)].astype(np.int64)
    kd = Keyed(pqv, st.s, st.n, values, valid)
    dev = torch.device("cuda", 0)
    q_t = torch.from_numpy(q).to(dev)
    src = torch.from_numpy(qkeys - 7).to(dev)
    qk_t = torch.zeros(nq, dtype=torch.int64, device=dev)
    r_t = torch.full((nq, k), -1, dtype=torch.int32, device=dev)
    d_t = torch.zeros((nq, k), dtype=torch.float32, device=dev)
    nf_t = torch.zeros(nq, dtype=torch.int32, device=dev)
    big = torch.zeros(1 << 24, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        for _ in range(20):
            big.add_(1.0)                   # work ahead of the keys on the stream
        torch.add(src, 7, out=qk_t)         # the keys are written on the stream ...
        st.s.topk_device(q_t.data_ptr(), nq, k, nprobe, r_t.data_ptr(), d_t.data_ptr(), nf_t.data_ptr(), sqrt_out=False,
                         stream=side.cuda_stream, keys=kd.keys, query_keys=qk_t.data_ptr())      # ... and read behind that write
    side.synchronize()
    exp = kd.y_device(q, qkeys, k, nprobe, False)
    _same((r_t.cpu().numpy().view(np.uint32), d_t.cpu().numpy(), nf_t.cpu().numpy().astype(np.uint32)), exp[:3], "stream order")
    kd.close()


def test_errors_and_lifetimes(pqv, oracle):
    """Case 9: the checks that need real handles; the column freed before the first search (every Keyed does that); searcher and
    keys freed in either order; keys of another searcher refused."""
    import ctypes as C
    from pq_vector_amd import _ffi
    st = Setup(pqv, oracle, 1500, 30, 6, seed=19)
    other = pqv.Searcher(pqv.Index.from_parts(30, st.centroids, st.lists), st.corpus)
    rng = np.random.default_rng(20)
    values, valid, ids = _column(rng, st.n, 3, np.int32, True)
    qkeys = _query_keys(rng, values, ids)[:5]
    kd = Keyed(pqv, st.s, st.n, values, valid)
    for call in (lambda: other.topk(st.queries, 5, 2, keys=kd.keys, query_keys=qkeys),
                 lambda: other.range_search(st.queries, 1.0, 2, keys=kd.keys, query_keys=qkeys),
                 lambda: _device(other, st.queries, 5, 2, False, keys=kd.keys, qkeys=qkeys)):
        with pytest.raises(pqv.PqvError, match="row keys belong to another searcher") as e:
            call()
        assert e.value.code == -1
    foreign = other.row_mask(np.ones(st.n, bool))
    with pytest.raises(pqv.PqvError, match="row mask belongs to another searcher"):
        st.s.topk(st.queries, 5, 2, keys=kd.keys, query_keys=qkeys, mask=foreign)
    foreign.close()
    lib, h = _ffi.lib(), C.c_void_p()
    fcol = pqv.Column.upload(np.zeros(st.n, np.float32))
    assert lib.pqv_row_keys_create(st.s._h, fcol._h, None, C.byref(h)) == -1
    assert b"key column must be PQV_COL_I32 or PQV_COL_I64" in lib.pqv_last_error() and not h.value
    short = pqv.Column.upload(np.zeros(st.n - 1, np.int64))
    with pytest.raises(pqv.PqvError, match=f"column has {st.n - 1} rows, the corpus has {st.n}"):
        st.s.row_keys(short)
    fcol.close(); short.close()
    q = st.queries[0]
    rows = np.zeros(5, np.uint32); dist = np.zeros(5, np.float32)
    rc = lib.pqv_topk_keyed(st.s._h, kd.keys._h, None, None, q.ctypes.data_as(_ffi.f32p), 1, 30, 5, 2, 0, 0, 1,
                            rows.ctypes.data_as(_ffi.u32p), dist.ctypes.data_as(_ffi.f32p), None, None)
    assert rc == -1 and b"query keys must not be NULL" in lib.pqv_last_error()
    # an attached column by name (attached without validity bytes)
    st.s.attach_column("tenant", values)
    by_name = st.s.row_keys("tenant")
    dense = Keyed(pqv, st.s, st.n, values, None)
    _same(st.s.topk(st.queries, 10, 3, keys=by_name, query_keys=qkeys), dense.y_topk(st.queries, qkeys, 10, 3), "keys of an attached column")
    by_name.close(); dense.close()
    # keys freed before their searcher: the searcher goes on
    kd.close()
    assert st.s.topk(st.queries, 3, 1)[2].tolist() == [3] * 5
    # ... and after it
    col = pqv.Column.upload(values, valid)
    late = other.row_keys(col)
    col.close()
    other.close()
    assert late.rows == st.n and late.dtype == _ffi.PQV_COL_I32
    late.close()


def test_two_submissions_are_bit_equal(shape):
    """Case 10."""
    st = shape
    rng = np.random.default_rng(91)
    values, valid, ids = _column(rng, st.n, 64, np.int64, True)
    qkeys = _query_keys(rng, values, ids)
    kd = Keyed(st.pqv, st.s, st.n, values, valid)
    for k, nprobe in ((10, 3), (300, st.kc)):
        _same(kd.topk(st.q7, qkeys, k, nprobe, metric=st.metric), kd.topk(st.q7, qkeys, k, nprobe, metric=st.metric), "topk twice")
        a, b = kd.device(st.q7, qkeys, k, nprobe, True, metric=st.metric), kd.device(st.q7, qkeys, k, nprobe, True, metric=st.metric)
        _same(a, b, "device twice")
    r = st.radius(3, st.metric)
    _same_range(kd.range(st.q7, qkeys, r, 3, metric=st.metric), kd.range(st.q7, qkeys, r, 3, metric=st.metric), "range twice")
    kd.close()
