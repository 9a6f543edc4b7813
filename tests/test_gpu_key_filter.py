"""Per-query key filters beyond equality on the GPU (pqv_key_filter: pqv_topk_filtered / pqv_topk_filtered_device /
pqv_range_search_filtered; Searcher.topk / topk_device / range_search with query_key_ranges= / query_key_sets=).

The yardstick is never the code under test: for every query of a filtered call it is ONE existing mask= call for that query
alone under searcher.row_mask(key_filter_ref.allowed_for(...)).  Rows, distance bits, n_found / n_within, n_candidates, tie flags
and lims must be equal.  (The one exception is the sub-batch case with its thousands of queries: there the queries that share
a filter share one masked call, as tests/test_gpu_keyed.py groups them, and a sample is also held to the per-query yardstick.)

Non-vacuity: every filter set built by _filters carries a broad filter (query 0), an empty one (query 1) and one that matches
only four PLANTED rows of the list nearest to query 2 (chosen on the CPU from the oracle's candidate order), so that in every
uncapped case the yardstick itself holds a query with n_found == 0, one with n_found == k and -- at k == 10; at k == 1 there
is no number between 0 and k -- one with 0 < n_found < k.  _nonvacuous asserts that on the yardstick's results."""
import collections

import numpy as np
import pytest

import key_filter_ref as kf
import mask_ref
from test_gpu_keyed import _same_range, _split_range
from test_gpu_mask import SHAPES, Setup, _bits, _same

pytestmark = pytest.mark.gpu

EMPTY = 0xFFFFFFFF
NQ = 7
PLANT = 10_000          # planted key values PLANT, PLANT + 2, PLANT + 4, PLANT + 6 (times the column's scale); ordinary ones lie in [-500, 500)

Flt = collections.namedtuple("Flt", "kind a b")      # the descriptor's arrays as Python ints: RANGE lo / hi [nq]; IN lims [nq + 1] / vals


def _sub(flt, idx):
    """the descriptor of the queries idx (a list) alone"""
    if flt.kind == kf.IN:
        lims, vals = [0], []
        for i in idx:
            vals += flt.b[flt.a[i]:flt.a[i + 1]]
            lims.append(len(vals))
        return Flt(kf.IN, lims, vals)
    return Flt(flt.kind, [flt.a[i] for i in idx], [flt.b[i] for i in idx] if flt.b is not None else None)


def _host_kw(flt):
    if flt.kind == kf.EQ:
        return {"query_keys": np.array(flt.a, np.int64)}
    if flt.kind == kf.RANGE:
        return {"query_key_ranges": (np.array(flt.a, np.int64), np.array(flt.b, np.int64))}
    return {"query_key_sets": [flt.b[flt.a[i]:flt.a[i + 1]] for i in range(len(flt.a) - 1)]}


def _device(s, q, k, nprobe, flags, mask=None, keys=None, flt=None, metric=0, max_candidates=0, poison=None):
    """topk_device with d2 output -> (rows, dist, n_found, n_candidates, tie flags or None).  poison (IN): values laid in front of
    and behind the values array on the device; the call gets the address of the first real value."""
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
    if flt is not None:
        front = list(poison) if poison is not None else []
        a_t = torch.from_numpy(np.array(flt.a, np.int64)).to(dev)                 # (lims: the same bits as uint64)
        b_t = torch.from_numpy(np.array(front + list(flt.b if flt.b is not None else []) + front + [0], np.int64)).to(dev)
        b_ptr = b_t.data_ptr() + 8 * len(front)
        kw["keys"] = keys
        if flt.kind == kf.EQ:
            kw["query_keys"] = a_t.data_ptr()
        elif flt.kind == kf.RANGE:
            kw["query_key_ranges"] = (a_t.data_ptr(), b_ptr)
        else:
            kw["query_key_sets"] = (a_t.data_ptr(), b_ptr)
    torch.cuda.synchronize()
    s.topk_device(q_t.data_ptr(), nq, k, nprobe, r_t.data_ptr(), d_t.data_ptr(), nf_t.data_ptr(), nc_t.data_ptr(), sqrt_out=False,
                  max_candidates=max_candidates, metric=metric, d_tie_flags=tf_t.data_ptr() if flags else 0, **kw)
    torch.cuda.synchronize()
    return (r_t.cpu().numpy().view(np.uint32), d_t.cpu().numpy(), nf_t.cpu().numpy().astype(np.uint32),
            nc_t.cpu().numpy().astype(np.uint64), tf_t.cpu().numpy() if flags else None)


class Filtered:
    """A key column over a searcher's rows, its RowKeys, and the yardstick: one masked call per query."""

    def __init__(self, pqv, s, n, values, valid=None, shared=None):
        self.pqv, self.s, self.values, self.valid, self.shared = pqv, s, values, valid, shared
        column = pqv.Column.upload(values, valid, device=0)
        self.keys = s.row_keys(column)
        assert self.keys.rows == n
        column.close()
        self.shared_mask = s.row_mask(shared) if shared is not None else None
        self._masks = {}

    def allowed(self, flt, i):
        return kf.allowed_for(self.values, self.valid, flt.kind, flt.a, flt.b, i, self.shared)

    def mask(self, flt, i):
        key = (id(flt), i)
        if key not in self._masks:
            self._masks[key] = (flt, self.s.row_mask(self.allowed(flt, i)))       # (flt is kept alive: its id stays its own)
        return self._masks[key][1]

    def close(self):
        for _, m in self._masks.values():
            m.close()
        if self.shared_mask is not None:
            self.shared_mask.close()
        self.keys.close()

    # --- the filtered calls
    def topk(self, q, flt, k, nprobe, **kw):
        return self.s.topk(q, k, nprobe, keys=self.keys, mask=self.shared_mask, **_host_kw(flt), **kw)

    def device(self, q, flt, k, nprobe, flags, **kw):
        return _device(self.s, q, k, nprobe, flags, mask=self.shared_mask, keys=self.keys, flt=flt, **kw)

    def range(self, q, flt, radius, nprobe, **kw):
        return _split_range(self.s.range_search(q, radius, nprobe, keys=self.keys, mask=self.shared_mask, **_host_kw(flt), **kw), len(q))

    # --- the yardstick: every query alone, under its own mask
    def y_topk(self, q, flt, k, nprobe, **kw):
        per = [[x[0] for x in self.s.topk(q[i:i + 1], k, nprobe, mask=self.mask(flt, i), **kw)] for i in range(len(q))]
        return tuple(np.stack([p[c] for p in per]) for c in range(4))

    def y_device(self, q, flt, k, nprobe, flags, **kw):
        n_out = 5 if flags else 4
        per = [[x[0] for x in _device(self.s, q[i:i + 1], k, nprobe, flags, mask=self.mask(flt, i), **kw)[:n_out]] for i in range(len(q))]
        return tuple(np.stack([p[c] for p in per]) for c in range(n_out)) + (() if flags else (None,))

    def y_range(self, q, flt, radius, nprobe, **kw):
        return [_split_range(self.s.range_search(q[i:i + 1], radius, nprobe, mask=self.mask(flt, i), **kw), 1)[0] for i in range(len(q))]


def _scale(dtype):
    return 1 if dtype == np.int32 else 2 ** 32 + 12345


def _column(rng, st, q, dtype, nulls, sorted_rows=False, shared=None):
    """-> (values [n], valid or None): ordinary values in [-500, 500) times the column's scale (int64: most beyond +-2^32) --
    sorted_rows: ascending with the row, eight rows per value -- and four planted rows of the list nearest to q[2], valid (and
    allowed by `shared`, changed in place) whatever the rest is."""
    n, sc = st.n, _scale(dtype)
    base = (np.arange(n) // 8) % 1000 - 500 if sorted_rows else rng.integers(-500, 500, n)
    values = (base.astype(np.int64) * sc).astype(dtype)
    valid = (rng.random(n) >= 1 / 8).astype(np.uint8) if nulls else None
    cand = np.asarray(st.oidx.candidate_rows(q[2], 1)).astype(np.int64)
    assert len(cand) >= 16
    planted = cand[[1, len(cand) // 3, len(cand) // 2, len(cand) - 1]]
    values[planted] = (np.array([0, 2, 4, 6]) + PLANT) * sc
    if valid is not None:
        valid[planted] = 1
    if shared is not None:
        shared[planted] = True
    return values, valid


def _filters(rng, values, kind, lens=(1, 63, 64, 65), twin=False):
    """The 7 filters of a call.  Queries 0 / 1 / 2: broad / empty / the planted rows only.
    RANGE, queries 3 .. 6: lo == hi on a present value; [INT64_MIN, INT64_MAX]; half open; bounds beyond +-2^31 ([2^40, 2^41]:
    nothing on an int32 column).
    IN, query 0 holds 1024 values, query 1 none, query 2 the planted values with absent ones on either side of each; queries
    3 .. 6: sets of lens values drawn from [-600, 600) (a third absent from the column, on both sides of present ones), the
    last one with INT64_MIN and INT64_MAX as members; twin: query 5 carries query 4's set."""
    sc = _scale(values.dtype.type)
    present = int(values[int(rng.integers(0, len(values)))])
    if kind == kf.RANGE:
        lo = [-250 * sc, 7, (PLANT - 1) * sc, present, kf.INT64_MIN, 100 * sc, 2 ** 40]
        hi = [249 * sc, 6, (PLANT + 7) * sc, present, kf.INT64_MAX, kf.INT64_MAX, 2 ** 41]
        return Flt(kf.RANGE, lo, hi)
    sets = [[v * sc for v in range(-1024, 1024, 2)], [], [(PLANT + d) * sc for d in range(-1, 8)]]
    for j, m in enumerate(lens):
        s = set(int(v) * sc for v in rng.choice(np.arange(-600, 600), size=m, replace=False))
        if j == len(lens) - 1 and m >= 3:
            s = set(sorted(s)[:m - 2]) | {kf.INT64_MIN, kf.INT64_MAX}
        if m == 1:
            s = {present}
        assert len(s) == m
        sets.append(sorted(s))
    if twin:
        sets[5] = list(sets[4])
    assert len(sets) == NQ and len(sets[0]) == kf.SET_MAX
    lims, vals = kf.sets_to_csr(sets)
    return Flt(kf.IN, [int(x) for x in lims], [int(x) for x in vals])


def _nonvacuous(nf, k, what):
    nf = np.asarray(nf).astype(np.int64)
    assert (nf == 0).any() and (nf == k).any(), f"vacuous case {what}: n_found {nf.tolist()}"
    if k > 1:
        assert ((nf > 0) & (nf < k)).any(), f"vacuous case {what}: n_found {nf.tolist()}"


def _check_all_entry_points(st, fd, q, flt, ks, nprobes, metric, what, nonvacuous=True):
    nc_unfiltered = st.s.topk(q, 1, max(nprobes), metric=metric)[3]
    for nprobe in nprobes:
        for k in ks:
            w = f"{what} k={k} nprobe={nprobe}"
            got, exp = fd.topk(q, flt, k, nprobe, metric=metric), fd.y_topk(q, flt, k, nprobe, metric=metric)
            if nonvacuous and k <= 10:
                _nonvacuous(exp[2], k, w)
            _same(got, exp, "topk " + w)
            assert (got[2] <= k).all()
            for flags in (False, True):
                got = fd.device(q, flt, k, nprobe, flags, metric=metric)
                exp = fd.y_device(q, flt, k, nprobe, flags, metric=metric)
                _same(got[:4], exp[:4], f"device flags={flags} " + w)
                if flags:
                    assert (got[4] == exp[4]).all(), "tie flags " + w
        r = st.radius(nprobe, metric)
        for max_results in (0, 7):
            _same_range(fd.range(q, flt, r, nprobe, max_results=max_results, metric=metric),
                        fd.y_range(q, flt, r, nprobe, max_results=max_results, metric=metric), f"range max_results={max_results} nprobe={nprobe} {what}")
    assert (fd.topk(q, flt, 1, max(nprobes), metric=metric)[3] == nc_unfiltered).all()      # n_candidates stays the unfiltered count


@pytest.fixture(scope="module", params=list(SHAPES))
def shape(request, pqv, oracle):
    c = SHAPES[request.param]
    st = Setup(pqv, oracle, c["n"], c["dim"], c["kc"], seed=11 + c["dim"])
    st.metric = c["metric"]
    st.q7 = np.random.default_rng(5 + c["dim"]).random((NQ, c["dim"]), dtype=np.float32)
    return st


@pytest.mark.parametrize("kind", [kf.RANGE, kf.IN], ids=["range", "in"])
@pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
@pytest.mark.parametrize("dtype", [np.int32, np.int64], ids=["i32", "i64"])
def test_filtered_calls_equal_one_masked_call_per_query(shape, dtype, nulls, kind):
    """Every entry point x I32 / I64 x with / without NULLs x RANGE / IN: k in {1, 10, 100, 300} (S = 1, 4, 16), nprobe in
    {1, 3, all}; topk, topk_device with and without tie flags, range_search with max_results in {0, 7}."""
    st = shape
    rng = np.random.default_rng(1000 * kind + 10 * st.dim + 2 * nulls + (dtype == np.int64))
    values, valid = _column(rng, st, st.q7, dtype, nulls)
    flt = _filters(rng, values, kind)
    fd = Filtered(st.pqv, st.s, st.n, values, valid)
    try:
        _check_all_entry_points(st, fd, st.q7, flt, (1, 10, 100, 300), (1, 3, st.kc), st.metric, "")
        rows, dist, nf, _ = fd.topk(st.q7, flt, 10, st.kc, metric=st.metric)
        empty = [1] + ([6] if kind == kf.RANGE and dtype == np.int32 else [])      # lo > hi / no values; [2^40, 2^41] on an int32 column
        for i in empty:
            assert nf[i] == 0 and (rows[i] == EMPTY).all() and np.isinf(dist[i]).all() and (dist[i] > 0).all()
        assert 1 <= nf[2] <= 4 and nf[0] == 10
        hit = fd.range(st.q7, flt, 1e30, st.kc, metric=st.metric)
        for i in empty:
            assert len(hit[i][0]) == 0 and hit[i][2] == 0
        assert hit[2][2] == 4                                                       # the planted rows, all valid
        if kind == kf.RANGE:                                                        # [INT64_MIN, INT64_MAX]: every valid row
            assert hit[4][2] == (st.n if valid is None else int(valid.sum()))
    finally:
        fd.close()


@pytest.mark.parametrize("sorted_rows", [False, True], ids=["random", "sorted"])
def test_range_edges_and_the_keyed_call(shape, sorted_rows):
    """RANGE edge cases on a random column and on one sorted by row (windows of all-ones / all-zeros runs): lo > hi, lo == hi,
    the full range, a half-open one, bounds beyond +-2^31 on an int32 column -- and lo == hi equals the existing query_keys= call
    bit for bit."""
    st = shape
    rng = np.random.default_rng(300 + st.dim + sorted_rows)
    values, valid = _column(rng, st, st.q7, np.int32, not sorted_rows, sorted_rows=sorted_rows)
    flt = _filters(rng, values, kf.RANGE)
    fd = Filtered(st.pqv, st.s, st.n, values, valid)
    try:
        _check_all_entry_points(st, fd, st.q7, flt, (10, 100), (1, st.kc), st.metric, f"sorted={sorted_rows}")
        qk = np.array([int(values[i]) for i in rng.integers(0, st.n, NQ)], np.int64)
        qk[1], qk[2], qk[6] = 777 * 1000, PLANT + 2, 2 ** 32 + int(qk[0])          # absent; one planted row; matches nothing, truncated it would
        same = Flt(kf.RANGE, qk.tolist(), qk.tolist())
        for k, nprobe in ((1, 1), (10, 3), (300, st.kc)):
            exp = st.s.topk(st.q7, k, nprobe, keys=fd.keys, query_keys=qk, metric=st.metric)
            if k <= 10:
                assert exp[2][1] == 0 and exp[2][6] == 0 and exp[2][2] == 1
            _same(fd.topk(st.q7, same, k, nprobe, metric=st.metric), exp, f"lo == hi against query_keys= k={k}")
            _same(fd.y_topk(st.q7, same, k, nprobe, metric=st.metric), exp, f"lo == hi yardstick k={k}")
            got = fd.device(st.q7, same, k, nprobe, True, metric=st.metric)
            _same(got, fd.device(st.q7, Flt(kf.EQ, qk.tolist(), None), k, nprobe, True, metric=st.metric), f"device lo == hi k={k}")
        r = st.radius(3, st.metric)
        _same_range(fd.range(st.q7, same, r, 3, metric=st.metric),
                    _split_range(st.s.range_search(st.q7, r, 3, keys=fd.keys, query_keys=qk, metric=st.metric), NQ), "range lo == hi")
    finally:
        fd.close()


def test_set_edges_and_the_keyed_call(shape):
    """IN edge cases: slice lengths 0, 1, 2, 63, 64, 65, 1 023 and 1 024 (the halving search's trip-count boundaries and the cap)
    over two calls, INT64_MIN / INT64_MAX as members, absent values on either side of present ones, two queries with one set, a
    device call whose values array lies between poison values that WOULD match, and singletons == the query_keys= call."""
    st = shape
    rng = np.random.default_rng(400 + st.dim)
    values, valid = _column(rng, st, st.q7, np.int64, True)
    fd = Filtered(st.pqv, st.s, st.n, values, valid)
    sc = _scale(np.int64)
    try:
        for lens, twin in (((1, 63, 64, 65), False), ((2, 1023, 1023, 3), True)):
            flt = _filters(rng, values, kf.IN, lens=lens, twin=twin)
            assert [flt.a[i + 1] - flt.a[i] for i in range(NQ)] == [1024, 0, 9] + list(lens)
            _check_all_entry_points(st, fd, st.q7, flt, (10, 100), (1, st.kc), st.metric, f"lens={lens}")
            if twin:
                assert flt.b[flt.a[4]:flt.a[5]] == flt.b[flt.a[5]:flt.a[6]]
            # poison: every ordinary value of the column in front of and behind the values array
            poison = [v * sc for v in range(-500, 500)]
            for k, nprobe in ((10, 3), (300, st.kc)):
                got = fd.device(st.q7, flt, k, nprobe, True, metric=st.metric, poison=poison)
                exp = fd.y_device(st.q7, flt, k, nprobe, True, metric=st.metric)
                _same(got, exp, f"poisoned values array k={k}")
                assert got[2][1] == 0                                              # the empty slice between two full ones
        qk = np.array([int(values[i]) for i in rng.integers(0, st.n, NQ)], np.int64)
        qk[1], qk[2], qk[3], qk[6] = 777 * sc, (PLANT + 2) * sc, kf.INT64_MAX, kf.INT64_MIN
        one = Flt(kf.IN, list(range(NQ + 1)), qk.tolist())
        for k, nprobe in ((1, 1), (10, 3), (300, st.kc)):
            exp = st.s.topk(st.q7, k, nprobe, keys=fd.keys, query_keys=qk, metric=st.metric)
            if k <= 10:
                assert exp[2][1] == 0 and exp[2][3] == 0 and exp[2][6] == 0 and exp[2][2] == 1
            _same(fd.topk(st.q7, one, k, nprobe, metric=st.metric), exp, f"singletons against query_keys= k={k}")
            _same(fd.y_topk(st.q7, one, k, nprobe, metric=st.metric), exp, f"singletons yardstick k={k}")
            _same(fd.device(st.q7, one, k, nprobe, True, metric=st.metric),
                  fd.device(st.q7, Flt(kf.EQ, qk.tolist(), None), k, nprobe, True, metric=st.metric), f"device singletons k={k}")
        r = st.radius(3, st.metric)
        _same_range(fd.range(st.q7, one, r, 3, metric=st.metric),
                    _split_range(st.s.range_search(st.q7, r, 3, keys=fd.keys, query_keys=qk, metric=st.metric), NQ), "range singletons")
    finally:
        fd.close()


@pytest.mark.parametrize("kind", [kf.RANGE, kf.IN], ids=["range", "in"])
def test_filtered_with_a_shared_mask(shape, kind):
    """filter AND one shared row mask == the masked call under M_q (which holds the shared mask)."""
    st = shape
    rng = np.random.default_rng(77 + kind + st.dim)
    shared = rng.random(st.n) < 0.5
    values, valid = _column(rng, st, st.q7, np.int32 if kind == kf.IN else np.int64, True, shared=shared)
    flt = _filters(rng, values, kind)
    fd = Filtered(st.pqv, st.s, st.n, values, valid, shared=shared)
    try:
        _check_all_entry_points(st, fd, st.q7, flt, (10, 300), (3, st.kc), st.metric, "shared 1/2")
    finally:
        fd.close()


def test_ties_follow_the_reference_heap_under_filters(pqv, oracle):
    """Tie-heavy integer data, dim 8: the host form's heap replay (RowFilter's range and set tests) and the device form's tie
    flags equal the yardstick's."""
    st = Setup(pqv, oracle, 3000, 8, 6, seed=4, integer=True)
    rng = np.random.default_rng(2)
    qs = rng.integers(0, 3, (3 * NQ, 8)).astype(np.float32)
    for kind, dtype, nulls in ((kf.RANGE, np.int64, True), (kf.IN, np.int32, False)):
        values, valid = _column(rng, st, qs, dtype, nulls)
        flt = _filters(rng, values, kind)
        fd = Filtered(pqv, st.s, st.n, values, valid)
        before = st.s.counters()["exact_replays"]
        flagged = 0
        for g in range(3):
            q = qs[g * NQ:(g + 1) * NQ]
            for k, nprobe in ((5, 2), (20, st.kc), (100, 3)):
                _same(fd.topk(q, flt, k, nprobe), fd.y_topk(q, flt, k, nprobe), f"tied host form k={k}")
                got, exp = fd.device(q, flt, k, nprobe, True), fd.y_device(q, flt, k, nprobe, True)
                _same(got[:4], exp[:4], f"tied device form k={k}")
                assert (got[4] == exp[4]).all()
                flagged += int(got[4].sum())
        assert flagged and st.s.counters()["exact_replays"] > before
        fd.close()


@pytest.mark.parametrize("kind", [kf.RANGE, kf.IN], ids=["range", "in"])
@pytest.mark.parametrize("name", ["4096x128", "1500x30", "2048x32-seq"])
def test_max_candidates_caps_before_the_filter(pqv, oracle, name, kind):
    """Plain searcher, max_candidates in {1, 100, just below the total}: capped first, then filtered; embeddings_fetched advances
    by the considered rows of the yardstick masks and candidate_rows by the uncapped totals, summed over the batch.  (A cap cuts
    the planted rows away: the non-vacuity condition is asserted on the uncapped call only.)"""
    c = SHAPES[name]
    st = Setup(pqv, oracle, c["n"], c["dim"], c["kc"], seed=21)
    metric = c["metric"]
    rng = np.random.default_rng(31 + kind)
    q = rng.random((NQ, c["dim"]), dtype=np.float32)
    values, valid = _column(rng, st, q, np.int32, True)
    flt = _filters(rng, values, kind)
    fd = Filtered(pqv, st.s, st.n, values, valid)
    cands = [st.oidx.candidate_rows(x, 3) for x in q]
    _nonvacuous(fd.y_topk(q, flt, 10, 3, metric=metric)[2], 10, "uncapped")
    for cap in (0, 1, 100, min(len(x) for x in cands) - 1):
        exp = [mask_ref.masked_topk(cands[i], fd.allowed(flt, i), st.data, q[i], 10, metric=metric, max_candidates=cap) for i in range(NQ)]
        cons, tot = sum(e[3] for e in exp), sum(e[2] for e in exp)
        before = st.s.counters()
        got = fd.topk(q, flt, 10, 3, max_candidates=cap, metric=metric, sqrt_out=False)
        after = st.s.counters()
        assert after["embeddings_fetched"] - before["embeddings_fetched"] == cons
        assert after["candidate_rows"] - before["candidate_rows"] == tot
        assert after["queries"] - before["queries"] == NQ
        _same(got, fd.y_topk(q, flt, 10, 3, max_candidates=cap, metric=metric, sqrt_out=False), f"capped topk {cap}")
        before = st.s.counters()
        dv = fd.device(q, flt, 10, 3, True, max_candidates=cap, metric=metric)
        after = st.s.counters()
        assert after["embeddings_fetched"] - before["embeddings_fetched"] == cons
        assert after["candidate_rows"] - before["candidate_rows"] == tot
        _same(dv[:4], fd.y_device(q, flt, 10, 3, True, max_candidates=cap, metric=metric)[:4], f"capped device {cap}")
        radius = 0.9 * float(np.sqrt(c["dim"] / 6.0))
        before = st.s.counters()
        rg = fd.range(q, flt, radius, 3, max_candidates=cap, metric=metric)
        after = st.s.counters()
        assert after["embeddings_fetched"] - before["embeddings_fetched"] == cons
        assert after["candidate_rows"] - before["candidate_rows"] == tot
        _same_range(rg, fd.y_range(q, flt, radius, 3, max_candidates=cap, metric=metric), f"capped range {cap}")
        for i in range(NQ):
            rr, rd, nw, nc = mask_ref.masked_range(cands[i], fd.allowed(flt, i), st.data, q[i], radius, metric=metric, max_candidates=cap)
            assert (rg[i][0] == rr).all() and (rg[i][1] == _bits(rd)).all() and rg[i][2:] == (nw, nc)
    fd.close()


def test_table_round_robin_quotas_come_before_the_filter(pqv, oracle):
    """Three files under PQV_TABLE_CAP_ROUND_ROBIN (tests/test_gpu_table_cap.py's set-up), keys over CORPUS rows."""
    from test_gpu_table import Table
    from test_gpu_table_cap import _selected
    rng = np.random.default_rng(12)
    t = Table(pqv, oracle, rng, [900, 1400, 500], [4, 6, 3], 32, gap=5, flags=pqv.PQV_TABLE_CAP_ROUND_ROBIN)
    n = len(t.data)
    q = rng.random((NQ, 32), dtype=np.float32)
    values = rng.integers(-500, 500, n).astype(np.int64) * _scale(np.int64)
    valid = (rng.random(n) >= 1 / 8).astype(np.uint8)
    planted = np.asarray(t.cand(q[2], 1)).astype(np.int64)[[0, 5, 11, 17]]         # (rows of query 2's nearest lists, one per file and more)
    values[planted] = (np.array([0, 2, 4, 6]) + PLANT) * _scale(np.int64)
    valid[planted] = 1
    fd = Filtered(pqv, t.s, n, values, valid)
    for kind in (kf.RANGE, kf.IN):
        flt = _filters(rng, values, kind)
        for nprobe in (1, 2):
            for cap in (0, 500, 2000):
                sels = [_selected(t, oracle, x, nprobe, cap)[0] if cap else t.cand(x, nprobe) for x in q]
                exp = [mask_ref.masked_topk(sels[i], fd.allowed(flt, i), t.data, q[i], 10) for i in range(NQ)]
                before = t.s.counters()
                got = fd.topk(q, flt, 10, nprobe, max_candidates=cap, sqrt_out=False)
                after = t.s.counters()
                assert after["embeddings_fetched"] - before["embeddings_fetched"] == sum(e[3] for e in exp)
                yard = fd.y_topk(q, flt, 10, nprobe, max_candidates=cap, sqrt_out=False)
                if not cap:
                    _nonvacuous(yard[2], 10, f"table nprobe={nprobe}")
                _same(got, yard, f"table topk cap={cap}")
                dv = fd.device(q, flt, 10, nprobe, True, max_candidates=cap)
                _same(dv[:4], fd.y_device(q, flt, 10, nprobe, True, max_candidates=cap)[:4], f"table device cap={cap}")
                for i, (rows, d2, _, _) in enumerate(exp):
                    m = int(got[2][i])
                    assert m == len(rows) and (got[0][i, :m] == rows).all() and (_bits(got[1][i, :m]) == _bits(d2)).all()
                    assert got[3][i] == len(t.cand(q[i], nprobe))
                _same_range(fd.range(q, flt, 2.0, nprobe, max_candidates=cap), fd.y_range(q, flt, 2.0, nprobe, max_candidates=cap),
                            f"table range cap={cap}")
    fd.close()


def test_beyond_the_kernel_lists(pqv, oracle):
    """k = 1500, and 1 100 probed lists, through the host forms (the filter in the replay); the device form is unsupported."""
    st = Setup(pqv, oracle, 2200, 8, 1100, seed=15)
    rng = np.random.default_rng(16)
    q = rng.random((NQ, 8), dtype=np.float32)
    values = (rng.integers(-500, 500, st.n)).astype(np.int32)
    valid = (rng.random(st.n) >= 1 / 8).astype(np.uint8)
    fd = Filtered(pqv, st.s, st.n, values, valid)
    for kind in (kf.RANGE, kf.IN):
        flt = _filters(rng, values, kind)
        for k, nprobe in ((10, 1100), (1500, 1100), (1500, 40)):
            before = st.s.counters()
            got = fd.topk(q, flt, k, nprobe, sqrt_out=False)
            after = st.s.counters()
            _same(got, fd.y_topk(q, flt, k, nprobe, sqrt_out=False), f"beyond: k={k} nprobe={nprobe}")
            cons = tot = 0
            for i in range(NQ):
                rows, d2, nc, ncons = mask_ref.masked_topk(st.oidx.candidate_rows(q[i], nprobe), fd.allowed(flt, i), st.data, q[i], k)
                n = int(got[2][i])
                assert n == len(rows) == min(k, ncons) and got[3][i] == nc and (got[0][i, n:] == EMPTY).all()
                if len(np.unique(_bits(d2))) == len(d2):
                    assert (got[0][i, :n] == rows).all() and (_bits(got[1][i, :n]) == _bits(d2)).all()
                cons += ncons; tot += nc
            assert after["embeddings_fetched"] - before["embeddings_fetched"] == cons
            assert after["candidate_rows"] - before["candidate_rows"] == tot
            with pytest.raises(pqv.PqvError) as e:
                fd.device(q, flt, k, nprobe, False)
            assert e.value.code == -5
        rg = fd.range(q, flt, 0.5, 1100)
        _same_range(rg, fd.y_range(q, flt, 0.5, 1100), "range over 1100 probed lists")
    fd.close()


def test_cosine_and_dot(pqv, oracle):
    """PQV_COSINE equals the masked cosine call; PQV_DOT is refused with the keyed calls' text."""
    c = SHAPES["4096x128"]
    st = Setup(pqv, oracle, c["n"], c["dim"], c["kc"], seed=41)
    rng = np.random.default_rng(42)
    q = rng.random((NQ, c["dim"]), dtype=np.float32) - 0.5
    values, valid = _column(rng, st, q, np.int64, True)
    fd = Filtered(pqv, st.s, st.n, values, valid)
    cos = pqv.PQV_COSINE
    for kind in (kf.RANGE, kf.IN):
        flt = _filters(rng, values, kind)
        for k, nprobe in ((1, 1), (10, 3), (300, st.kc)):
            _same(fd.topk(q, flt, k, nprobe, metric=cos), fd.y_topk(q, flt, k, nprobe, metric=cos), f"cosine topk k={k}")
            got, exp = fd.device(q, flt, k, nprobe, True, metric=cos), fd.y_device(q, flt, k, nprobe, True, metric=cos)
            _same(got[:4], exp[:4], f"cosine device k={k}")
            assert (got[4] == exp[4]).all()
        radius = float(fd.topk(q, flt, 10, 3, metric=cos)[1][0, 5])
        assert np.isfinite(radius)
        _same_range(fd.range(q, flt, radius, 3, metric=cos), fd.y_range(q, flt, radius, 3, metric=cos), "cosine range")
        for call in (lambda: fd.topk(q, flt, 10, 3, metric=pqv.PQV_DOT), lambda: fd.device(q, flt, 10, 3, False, metric=pqv.PQV_DOT),
                     lambda: fd.range(q, flt, 1.0, 3, metric=pqv.PQV_DOT)):
            with pytest.raises(pqv.PqvError, match="PQV_DOT is not supported by keyed and distinct calls") as e:
                call()
            assert e.value.code == -5
    fd.close()


def test_host_sub_batches_slice_and_rebase_the_filters(pqv, oracle):
    """One host call of more queries than one sub-batch of pqv_topk_impl holds (tests/test_gpu_keyed.py's configuration and its
    restatement of the bound): eight distinct filters cycle over the queries, sets of different lengths, so the second sub-batch
    is right only if lo / hi were sliced and lims rebased.  Yardstick: one masked call per distinct filter over its queries,
    and the per-query yardstick for seven queries around the cut."""
    c = SHAPES["4096x128"]
    st = Setup(pqv, oracle, c["n"], c["dim"], c["kc"], seed=51)
    k, nprobe, dim = 300, st.kc, c["dim"]
    per_query = nprobe * 4 * (k + 1) * 12 + 4 * 64 * 12 + 8192 * 12 + nprobe * (dim + 32) + dim * 4 + 1
    batch = (1 << 30) // per_query
    nq = batch + batch // 2
    assert 2000 < batch < 8000
    rng = np.random.default_rng(52)
    q = rng.random((nq, dim), dtype=np.float32)
    values, valid = _column(rng, st, q, np.int32, True)
    fd = Filtered(pqv, st.s, st.n, values, valid)
    which = np.arange(nq) % 8
    around = list(range(batch - 3, batch + 4))
    for kind in (kf.RANGE, kf.IN):
        if kind == kf.RANGE:
            lo8, hi8 = [-500, 0, 5, PLANT, -100, 499, 300, kf.INT64_MIN], [-1, 499, 4, PLANT + 6, -90, 499, kf.INT64_MAX, -400]
            flt = Flt(kf.RANGE, [lo8[w] for w in which], [hi8[w] for w in which])
        else:
            sets8 = [sorted(int(v) for v in rng.choice(np.arange(-600, 600), size=m, replace=False)) for m in (300, 0, 1, 2, 63, 64, 65, 7)]
            lims, vals = kf.sets_to_csr([sets8[w] for w in which])
            flt = Flt(kf.IN, [int(x) for x in lims], [int(x) for x in vals])
        got = fd.topk(q, flt, k, nprobe)
        rg = fd.range(q[batch - 100:batch + 100], _sub(flt, list(range(batch - 100, batch + 100))), st.radius(1), 1)
        for w in range(8):
            idx = np.flatnonzero(which == w)
            m = fd.mask(flt, int(idx[0]))
            _same(tuple(x[idx] for x in got), st.s.topk(q[idx], k, nprobe, mask=m), f"sub-batched host call, filter {w}")
            sel = [i for i in range(batch - 100, batch + 100) if which[i] == w]
            _same_range([rg[i - (batch - 100)] for i in sel], _split_range(st.s.range_search(q[sel], st.radius(1), 1, mask=m), len(sel)), "range")
        _same(tuple(x[around] for x in got), fd.y_topk(q[around], _sub(flt, around), k, nprobe), "around the cut")
        assert (got[2][which == (1 if kind == kf.RANGE else 0)] > 0).all()
    fd.close()


def test_filter_arrays_are_read_in_stream_order(pqv, oracle):
    """The filter arrays are written by torch ops on a side stream and the filtered device call is enqueued on that stream with
    no synchronisation between."""
    import torch
    c = SHAPES["4096x128"]
    st = Setup(pqv, oracle, c["n"], c["dim"], c["kc"], seed=61)
    rng = np.random.default_rng(62)
    q = rng.random((NQ, c["dim"]), dtype=np.float32)
    values, valid = _column(rng, st, q, np.int64, False)
    fd = Filtered(pqv, st.s, st.n, values, valid)
    k, nprobe = 10, 3
    dev = torch.device("cuda", 0)
    q_t = torch.from_numpy(q).to(dev)
    big = torch.zeros(1 << 24, dtype=torch.float32, device=dev)
    side = torch.cuda.Stream(device=dev)
    for kind in (kf.RANGE, kf.IN):
        flt = _filters(rng, values, kind)
        src_a = torch.from_numpy(np.array(flt.a, np.int64) - 7).to(dev)
        src_b = torch.from_numpy(np.array(flt.b + [0], np.int64)).to(dev)
        a_t, b_t = torch.zeros_like(src_a), torch.full_like(src_b, 123)
        r_t = torch.full((NQ, k), -1, dtype=torch.int32, device=dev)
        d_t = torch.zeros((NQ, k), dtype=torch.float32, device=dev)
        nf_t = torch.zeros(NQ, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for _ in range(20):
                big.add_(1.0)                   # work ahead of the filter arrays on the stream
            torch.add(src_a, 7, out=a_t)        # the arrays are written on the stream ...
            b_t.copy_(src_b)
            kw = {"query_key_ranges" if kind == kf.RANGE else "query_key_sets": (a_t.data_ptr(), b_t.data_ptr())}
            st.s.topk_device(q_t.data_ptr(), NQ, k, nprobe, r_t.data_ptr(), d_t.data_ptr(), nf_t.data_ptr(), sqrt_out=False,
                             stream=side.cuda_stream, keys=fd.keys, **kw)      # ... and read behind those writes
        side.synchronize()
        exp = fd.y_device(q, flt, k, nprobe, False)
        _nonvacuous(exp[2], k, "stream order")
        _same((r_t.cpu().numpy().view(np.uint32), d_t.cpu().numpy(), nf_t.cpu().numpy().astype(np.uint32)), exp[:3], "stream order")
    fd.close()


def test_errors_and_lifetimes(pqv, oracle):
    """The checks that need real handles, in their order behind the descriptor's; searcher and keys freed in either order."""
    st = Setup(pqv, oracle, 1500, 30, 6, seed=19)
    other = pqv.Searcher(pqv.Index.from_parts(30, st.centroids, st.lists), st.corpus)
    rng = np.random.default_rng(20)
    q = rng.random((NQ, 30), dtype=np.float32)
    values, valid = _column(rng, st, q, np.int32, True)
    fd = Filtered(pqv, st.s, st.n, values, valid)
    for kind in (kf.RANGE, kf.IN):
        flt = _filters(rng, values, kind)
        for call in (lambda: other.topk(q, 5, 2, keys=fd.keys, **_host_kw(flt)), lambda: other.range_search(q, 1.0, 2, keys=fd.keys, **_host_kw(flt)),
                     lambda: _device(other, q, 5, 2, False, keys=fd.keys, flt=flt)):
            with pytest.raises(pqv.PqvError, match="row keys belong to another searcher") as e:
                call()
            assert e.value.code == -1
        foreign = other.row_mask(np.ones(st.n, bool))
        with pytest.raises(pqv.PqvError, match="row mask belongs to another searcher"):
            st.s.topk(q, 5, 2, keys=fd.keys, mask=foreign, **_host_kw(flt))
        foreign.close()
        with pytest.raises(pqv.PqvError, match="Query dimension mismatch"):
            st.s.topk(np.ascontiguousarray(q[:, :29]), 5, 2, keys=fd.keys, **_host_kw(flt))
    # keys freed before their searcher: the searcher goes on; and after it
    flt = _filters(rng, values, kf.IN)
    exp = fd.y_topk(q, flt, 10, 3)
    fd.keys.close()
    assert st.s.topk(q, 3, 1)[2].tolist() == [3] * NQ
    col = pqv.Column.upload(values, valid)
    late = other.row_keys(col)
    col.close()
    _same(other.topk(q, 10, 3, keys=late, **_host_kw(flt)), exp, "the same lists, another searcher's keys")
    other.close()
    assert late.rows == st.n
    late.close()
    fd.keys = st.s.row_keys(pqv.Column.upload(values, valid))
    fd.close()


@pytest.mark.parametrize("kind", [kf.RANGE, kf.IN], ids=["range", "in"])
def test_two_submissions_are_bit_equal(shape, kind):
    st = shape
    rng = np.random.default_rng(91 + kind)
    values, valid = _column(rng, st, st.q7, np.int64, True)
    flt = _filters(rng, values, kind)
    fd = Filtered(st.pqv, st.s, st.n, values, valid)
    for k, nprobe in ((10, 3), (300, st.kc)):
        a = fd.topk(st.q7, flt, k, nprobe, metric=st.metric)
        if k <= 10:
            _nonvacuous(fd.y_topk(st.q7, flt, k, nprobe, metric=st.metric)[2], k, "twice")
        _same(a, fd.topk(st.q7, flt, k, nprobe, metric=st.metric), "topk twice")
        a, b = fd.device(st.q7, flt, k, nprobe, True, metric=st.metric), fd.device(st.q7, flt, k, nprobe, True, metric=st.metric)
        _same(a, b, "device twice")
    r = st.radius(3, st.metric)
    _same_range(fd.range(st.q7, flt, r, 3, metric=st.metric), fd.range(st.q7, flt, r, 3, metric=st.metric), "range twice")
    fd.close()
