"""Grouped top-k on the GPU (pqv_topk_grouped / pqv_topk_grouped_device): up to m rows of each of the k nearest groups.

The yardstick everywhere is the same searcher's EXISTING range search: range_search(q, +inf, nprobe, sqrt_out=False, mask=key
validity AND shared mask) returns the considered rows sorted by (d2, position) -- the sequence S of pqv.h -- and numpy ranks the key
values by their first row in S, keeps k, and m rows of each (tests/grouped_ref.py: group_sorted).  Rows, distance bits, group
keys, group_rows, n_found and n_candidates must be equal, on the host and the device form, whose outputs start as garbage.
grouped_ref / distinct_ref over the oracle's candidates are a second opinion."""
import numpy as np
import pytest

import distinct_ref
import grouped_ref
from test_gpu_distinct import Distinct
from test_gpu_mask import SHAPES, Setup, _bits

pytestmark = pytest.mark.gpu

EMPTY = 0xFFFFFFFF
# (k, m): k * m = 2 and 15 (S = 1), 64 (its last entry), 65 (S = 4, its first), 256 (its last), 264 (S = 16), 1024 (its last)
KMS = ((1, 2), (5, 3), (16, 4), (13, 5), (64, 4), (33, 8), (128, 8))
UNSUPPORTED = "pqv_topk_grouped_device takes k \\* group_size <= 1024 and at most 1024 probed lists per query"


def _device(s, q, k, m, nprobe, keys, mask=None, metric=0, max_candidates=0, sqrt_out=False):
    """topk_grouped_device -> (rows, dist, group keys, group_rows, n_found, n_candidates); the outputs start as garbage"""
    import torch
    dev = torch.device("cuda", 0)
    q_t = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(dev)
    nq = len(q)
    r_t = torch.full((nq, k, m), 5, dtype=torch.int32, device=dev)
    d_t = torch.full((nq, k, m), -1.0, dtype=torch.float32, device=dev)
    g_t = torch.full((nq, k), 77, dtype=torch.int64, device=dev)
    c_t = torch.full((nq, k), 99, dtype=torch.int32, device=dev)
    nf_t = torch.full((nq,), 9, dtype=torch.int32, device=dev)
    nc_t = torch.full((nq,), 9, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    s.topk_grouped_device(q_t.data_ptr(), nq, k, m, nprobe, keys, r_t.data_ptr(), d_t.data_ptr(), g_t.data_ptr(), c_t.data_ptr(),
                          nf_t.data_ptr(), nc_t.data_ptr(), mask=mask, max_candidates=max_candidates, metric=metric, sqrt_out=sqrt_out)
    torch.cuda.synchronize()
    return (r_t.cpu().numpy().view(np.uint32), d_t.cpu().numpy(), g_t.cpu().numpy(), c_t.cpu().numpy().view(np.uint32),
            nf_t.cpu().numpy().astype(np.uint32), nc_t.cpu().numpy().astype(np.uint64))


class Grouped(Distinct):
    """test_gpu_distinct's group column, keys, shared mask and yardstick mask; the sorted considered sequence is computed once per
    (queries, nprobe, metric, cap) and shared by every (k, m) checked against it."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._seq = {}

    def sequence(self, q, nprobe, metric=0, max_candidates=0):
        key = (q.tobytes(), nprobe, metric, max_candidates)
        if key not in self._seq:
            lims, rows, dist, _, nc = self.s.range_search(q, np.inf, nprobe, sqrt_out=False, mask=self.ymask, metric=metric,
                                                          max_candidates=max_candidates)
            self._seq[key] = (lims, rows, dist, nc)
        return self._seq[key]

    def yardstick(self, q, k, m, nprobe, metric=0, max_candidates=0):
        lims, rows, dist, nc = self.sequence(q, nprobe, metric, max_candidates)
        nq = len(q)
        o_r = np.empty((nq, k, m), np.uint32); o_d = np.empty((nq, k, m), np.float32)
        o_g = np.empty((nq, k), np.int64); o_c = np.empty((nq, k), np.uint32); o_n = np.zeros(nq, np.uint32)
        for i in range(nq):
            a, b = int(lims[i]), int(lims[i + 1])
            o_r[i], o_d[i], o_g[i], o_c[i], o_n[i] = grouped_ref.group_sorted(rows[a:b], dist[a:b], self.values, k, m)
        return o_r, o_d, o_g, o_c, o_n, nc

    def host(self, q, k, m, nprobe, metric=0, max_candidates=0):
        return self.s.topk_grouped(q, k, m, nprobe, self.keys, mask=self.shared_mask, metric=metric, max_candidates=max_candidates,
                                   sqrt_out=False)

    def device(self, q, k, m, nprobe, metric=0, max_candidates=0):
        return _device(self.s, q, k, m, nprobe, self.keys, mask=self.shared_mask, metric=metric, max_candidates=max_candidates)

    def check(self, q, k, m, nprobe, what="", forms=("host", "device"), **kw):
        exp = self.yardstick(q, k, m, nprobe, **kw)
        for form in forms:
            got = getattr(self, form)(q, k, m, nprobe, **kw)
            w = f"{form} k={k} m={m} nprobe={nprobe} {what}"
            assert got[0].shape == (len(q), k, m) and got[3].shape == (len(q), k), "shapes " + w
            assert (got[4] == exp[4]).all(), "n_found " + w
            assert (got[2] == exp[2]).all(), "group keys " + w
            assert (got[3] == exp[3]).all(), "group_rows " + w
            assert (got[0] == exp[0]).all(), "rows " + w
            assert (_bits(got[1]) == _bits(exp[1])).all(), "distance bits " + w
            assert (got[5] == exp[5]).all(), "n_candidates " + w
        return exp


@pytest.fixture(scope="module", params=list(SHAPES))
def shape(request, pqv, oracle):
    c = SHAPES[request.param]
    st = Setup(pqv, oracle, c["n"], c["dim"], c["kc"], seed=11 + c["dim"])
    st.metric = c["metric"]
    return st


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_every_shape_equals_the_grouped_range_search(pqv, shape, dtype):
    """Case 1: about 16 rows per key -- a group's rows fall into the same tile, other waves, other blocks and other lists."""
    st = shape
    values = st.rng.integers(0, st.n // 16, st.n).astype(dtype)
    d = Grouped(pqv, st.s, st.n, values)
    try:
        for nprobe in (1, 3, st.kc):
            for k, m in KMS:
                exp = d.check(st.queries, k, m, nprobe, metric=st.metric)
                assert (exp[4] == np.minimum(k, [len(np.unique(values[st.oidx.candidate_rows(q, nprobe)])) for q in st.queries])).all()
            assert exp[3].max() > 1                      # (groups of several rows were returned)
        # the second opinion: the restatements over the oracle's candidates
        for q in st.queries[:2]:
            r, d2, g, c, nf, nc, _ = grouped_ref.grouped_topk(st.oidx.candidate_rows(q, 3), values, None, None, st.data, q, 13, 5,
                                                              metric=st.metric)
            got = d.host(q.reshape(1, -1), 13, 5, 3, metric=st.metric)
            assert int(got[4][0]) == nf and (got[0][0] == r).all() and (_bits(got[1][0]) == _bits(d2)).all()
            assert (got[2][0] == g).all() and (got[3][0] == c).all() and got[5][0] == nc
            rd = distinct_ref.distinct_topk(st.oidx.candidate_rows(q, 3), values, None, None, st.data, q, 13, metric=st.metric)
            assert (got[0][0, :nf, 0] == rd[0]).all() and (got[2][0, :nf] == rd[2]).all()
    finally:
        d.close()


def test_group_size_one_is_the_distinct_call(pqv, shape):
    """Case 2: m = 1 returns what topk_distinct returns, padding included, and group_rows = 1 per found group."""
    from test_gpu_distinct import _device as distinct_device
    st = shape
    values = st.rng.integers(0, st.n // 16, st.n).astype(np.int64)
    valid = (st.rng.random(st.n) >= 0.3).astype(np.uint8)
    d = Grouped(pqv, st.s, st.n, values, valid, np.isin(values, np.arange(40)))       # (at most 40 groups: k = 65 and 200 are padded)
    try:
        for k, nprobe in ((1, 1), (65, 3), (200, st.kc)):
            for exp, got in ((d.s.topk_distinct(st.queries, k, nprobe, d.keys, mask=d.shared_mask, metric=st.metric, sqrt_out=False),
                              d.host(st.queries, k, 1, nprobe, metric=st.metric)),
                             (distinct_device(d.s, st.queries, k, nprobe, d.keys, mask=d.shared_mask, metric=st.metric),
                              d.device(st.queries, k, 1, nprobe, metric=st.metric))):
                assert (got[0][:, :, 0] == exp[0]).all() and (_bits(got[1][:, :, 0]) == _bits(exp[1])).all()
                assert (got[2] == exp[2]).all() and (got[4] == exp[3]).all() and (got[5] == exp[4]).all()
                assert (got[3] == (np.arange(k)[None, :] < exp[3][:, None])).all()
            if k > 40:
                assert (exp[3] < k).all()
    finally:
        d.close()


def test_all_keys_distinct_is_the_masked_top_k_in_slot_0(pqv, shape):
    """Case 3: bit-equal to topk_device under an all-ones mask in slot i = 0; every group has one row."""
    from test_gpu_mask import _device as masked_device
    st = shape
    d = Grouped(pqv, st.s, st.n, st.rng.permutation(st.n).astype(np.int64) - st.n // 2)
    ones = st.s.row_mask(np.ones(st.n, bool))
    try:
        for (k, m), nprobe in (((1, 2), 1), ((64, 4), 3), ((128, 8), st.kc)):
            exp = masked_device(st.s, st.queries, k, nprobe, False, mask=ones, metric=st.metric)
            for got in (d.host(st.queries, k, m, nprobe, metric=st.metric), d.device(st.queries, k, m, nprobe, metric=st.metric)):
                assert (got[0][:, :, 0] == exp[0]).all() and (_bits(got[1][:, :, 0]) == _bits(exp[1])).all() and (got[4] == exp[2]).all()
                assert (got[5] == exp[3]).all()
                assert (got[0][:, :, 1:] == EMPTY).all() and np.isposinf(got[1][:, :, 1:]).all()
                assert (got[3] == (exp[0] != EMPTY)).all()
                found = exp[0] != EMPTY
                assert (got[2][found] == d.values[exp[0][found].astype(np.int64)]).all() and (got[2][~found] == 0).all()
    finally:
        ones.close(); d.close()


def test_integer_data_ties_follow_d2_then_position(pqv, oracle):
    """Case 4: whole distance classes tie: the groups' ranks and the rows inside a group follow (d2, position)."""
    st = Setup(pqv, oracle, 3000, 8, 6, seed=4, integer=True)
    q = np.random.default_rng(2).integers(0, 3, (9, 8)).astype(np.float32)
    d = Grouped(pqv, st.s, st.n, st.rng.integers(0, st.n // 16, st.n).astype(np.int64))
    try:
        for (k, m), nprobe in (((5, 3), 2), ((33, 8), st.kc), ((128, 8), 3)):
            exp = d.check(q, k, m, nprobe)
            if k >= 33:      # (d2 is an integer <= 32: rows of one group must tie)
                assert any(len(np.unique(_bits(exp[1][i, g, :c]))) < c for i in range(len(q)) for g, c in enumerate(exp[3][i]) if c > 1)
        r, d2, g, c, nf, _, _ = grouped_ref.grouped_topk(st.oidx.candidate_rows(q[0], 2), d.values, None, None, st.data, q[0], 33, 8)
        got = d.host(q[:1], 33, 8, 2)
        assert (got[0][0] == r).all() and (_bits(got[1][0]) == _bits(d2)).all() and (got[2][0] == g).all() and (got[3][0] == c).all()
    finally:
        d.close()


@pytest.mark.parametrize("kind", ["high-word", "low-word", "negative", "zero"])
def test_wide_keys_are_compared_in_full(pqv, oracle, kind):
    """Case 5: I64 keys that differ only in the high word / only in the low word, negative keys (a half-width or unsigned compare
    in the set lookup merges or loses groups), and a real key 0 with n_found < k: the padding's 0 is no group."""
    st = Setup(pqv, oracle, 4096, 128, 8, seed=23)
    g = st.rng.integers(0, st.n // 16, st.n).astype(np.int64)
    if kind == "zero":
        for dtype in (np.int32, np.int64):
            d = Grouped(pqv, st.s, st.n, (g % 3).astype(dtype) - 1)           # the groups -1, 0, 1
            try:
                for got in (d.check(st.queries, 5, 3, 3, kind), d.host(st.queries, 5, 3, 3), d.device(st.queries, 5, 3, 3)):
                    assert (got[4] == 3).all() and (np.sort(got[2][:, :3], axis=1) == [-1, 0, 1]).all()
                    assert (got[3][:, :3] == 3).all() and (got[3][:, 3:] == 0).all() and (got[2][:, 3:] == 0).all()
                    assert (got[0][:, 3:] == EMPTY).all() and np.isposinf(got[1][:, 3:]).all()
            finally:
                d.close()
        return
    values = {"high-word": (g << 32) + 7, "low-word": (5 << 32) + g, "negative": -(g * (2 ** 32 + 12345)) - 1}[kind]
    d = Grouped(pqv, st.s, st.n, values)
    try:
        for k, m in ((5, 3), (13, 5)):
            d.check(st.queries, k, m, 3, kind)
    finally:
        d.close()
    if kind == "negative":       # ... and negative I32 keys are sign-extended for the lookup and come back so
        d = Grouped(pqv, st.s, st.n, (-g - 1).astype(np.int32))
        try:
            exp = d.check(st.queries, 13, 5, 3, "negative i32")
            assert (exp[2][exp[3] != 0] < 0).all()
        finally:
            d.close()


def test_groups_laid_out_by_list_position(pqv, oracle):
    """Case 6: key = list position // 3: a group's rows are neighbours in a list, so groups straddle the 64-position windows, the
    waves' ranges and the row blocks (none of which is a multiple of 3 apart from a multiple of 3).  m = 8 is larger than every
    group."""
    st = Setup(pqv, oracle, 4096, 128, 8, seed=29)
    order = np.concatenate([np.asarray(l, np.int64) for l in st.lists])
    values = np.empty(st.n, np.int64)
    values[order] = np.arange(st.n) // 3
    d = Grouped(pqv, st.s, st.n, values)
    try:
        for (k, m), nprobe in (((5, 3), 1), ((64, 4), 3), ((33, 8), st.kc), ((128, 8), 3)):
            exp = d.check(st.queries, k, m, nprobe, "position // 3")
            assert exp[3].max() == 3 and (exp[4] == k).all()
    finally:
        d.close()


def test_null_keys_and_a_shared_mask(pqv, shape):
    """Case 7: about 30 % NULL keys and a shared mask with p = 0.5; a mask that leaves fewer than k groups; one that leaves none."""
    st = shape
    values = st.rng.integers(0, st.n // 16, st.n).astype(np.int32)
    valid = (st.rng.random(st.n) >= 0.3).astype(np.uint8)
    shared = st.rng.random(st.n) < 0.5
    d = Grouped(pqv, st.s, st.n, values, valid, shared)
    try:
        for k, m in ((5, 3), (13, 5), (33, 8)):
            exp = d.check(st.queries, k, m, 3, metric=st.metric)
            found = exp[0][exp[0] != EMPTY].astype(np.int64)
            assert d.allowed[found].all()                     # no NULL-key row, no masked row
    finally:
        d.close()
    d = Grouped(pqv, st.s, st.n, values, valid, np.isin(values, [1, 2, 3]))
    try:
        exp = d.check(st.queries, 13, 5, st.kc, metric=st.metric)
        assert (exp[4] <= 3).all() and exp[4].max() > 0
    finally:
        d.close()
    d = Grouped(pqv, st.s, st.n, values, valid, np.zeros(st.n, bool))
    try:
        exp = d.check(st.queries, 5, 3, 3, metric=st.metric)
        assert (exp[4] == 0).all() and (exp[0] == EMPTY).all() and (exp[3] == 0).all()
    finally:
        d.close()


@pytest.mark.parametrize("name", ["4096x128", "1500x30"])
def test_max_candidates_cuts_before_the_groups(pqv, oracle, name):
    """Case 8: the cap falls inside the second probed list, and inside the first."""
    c = SHAPES[name]
    st = Setup(pqv, oracle, c["n"], c["dim"], c["kc"], seed=21)
    values = st.rng.integers(0, st.n // 16, st.n).astype(np.int64)
    valid = (st.rng.random(st.n) >= 0.3).astype(np.uint8)
    d = Grouped(pqv, st.s, st.n, values, valid)
    try:
        for q in st.queries[:3]:
            first = len(st.lists[int(st.oidx.find_closest_centroids(q, 1)[0])])
            for cap in (first + 100, 37):
                q1 = q.reshape(1, -1)
                exp = d.check(q1, 13, 5, 3, f"cap={cap}", max_candidates=cap)
                r, d2, g, cnt, nf, nc, _ = grouped_ref.grouped_topk(st.oidx.candidate_rows(q, 3), values, valid, None, st.data, q, 13, 5,
                                                                    max_candidates=cap)
                assert int(exp[4][0]) == nf and (exp[0][0] == r).all() and (_bits(exp[1][0]) == _bits(d2)).all() and exp[5][0] == nc
                assert (exp[3][0] == cnt).all()
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
    d = Grouped(pqv, t.s, n, values, None, shared)
    queries = rng.random((4, 32), dtype=np.float32)
    try:
        for nprobe in (1, 2):
            for cap in (0, 500):
                d.check(queries, 5, 3, nprobe, f"cap={cap}", max_candidates=cap)
                d.check(queries, 13, 5, nprobe, f"cap={cap}", max_candidates=cap)
                q = queries[0]
                cand = t.cand(q, nprobe)
                sel = _selected(t, oracle, q, nprobe, cap)[0] if cap else cand
                r, _, g, cnt, nf, _, _ = grouped_ref.grouped_topk(sel, values, None, shared, t.data, q, 5, 3)
                got = d.host(q.reshape(1, -1), 5, 3, nprobe, max_candidates=cap)
                assert int(got[4][0]) == nf and (got[0][0] == r).all() and (got[2][0] == g).all() and (got[3][0] == cnt).all()
                assert got[5][0] == len(cand)
    finally:
        d.close()


def test_cosine(pqv, oracle):
    """Case 10: PQV_COSINE through the cosine layout: the halved distances of the cosine range search, grouped."""
    st = Setup(pqv, oracle, 2048, 256, 4, seed=33)
    d = Grouped(pqv, st.s, st.n, st.rng.integers(0, st.n // 16, st.n).astype(np.int32), (st.rng.random(st.n) >= 0.3).astype(np.uint8))
    try:
        for k, m in ((5, 3), (33, 8)):
            d.check(st.queries, k, m, 2, "cosine", metric=pqv.PQV_COSINE)
    finally:
        d.close()


def test_dot_is_unsupported(pqv, oracle):
    """Case 11."""
    st = Setup(pqv, oracle, 1500, 30, 6, seed=19)
    d = Grouped(pqv, st.s, st.n, np.arange(st.n, dtype=np.int32) // 4)
    try:
        for call in (d.host, d.device):
            with pytest.raises(pqv.PqvError, match="PQV_DOT is not supported by keyed and distinct calls") as e:
                call(st.queries, 5, 3, 2, metric=pqv.PQV_DOT)
            assert e.value.code == -5
    finally:
        d.close()


def test_counters(pqv, oracle):
    """Case 12: queries and candidate_rows advance once per query, not once per pass; embeddings_fetched by the considered rows plus
    the rows the second pass evaluates -- the considered rows of the selected groups."""
    import mask_ref
    st = Setup(pqv, oracle, 4096, 128, 8, seed=17)
    values = st.rng.integers(0, st.n // 16, st.n).astype(np.int64)
    valid = (st.rng.random(st.n) >= 0.3).astype(np.uint8)
    d = Grouped(pqv, st.s, st.n, values, valid, st.rng.random(st.n) < 0.5)
    cap, k, m = 700, 10, 3
    try:
        exp = d.yardstick(st.queries, k, m, 3, max_candidates=cap)
        cons = second = 0
        for i, q in enumerate(st.queries):
            rows = mask_ref.considered(st.oidx.candidate_rows(q, 3), d.allowed, cap)[0]
            cons += len(rows)
            second += int(np.isin(values[rows.astype(np.int64)], exp[2][i, :int(exp[4][i])]).sum())
        assert 0 < second < cons
        tot = sum(len(st.oidx.candidate_rows(q, 3)) for q in st.queries)
        for call in (d.host, d.device):
            before = st.s.counters()
            call(st.queries, k, m, 3, max_candidates=cap)
            after = st.s.counters()
            assert after["embeddings_fetched"] - before["embeddings_fetched"] == cons + second
            assert after["candidate_rows"] - before["candidate_rows"] == tot
            assert after["queries"] - before["queries"] == len(st.queries)
    finally:
        d.close()


def test_beyond_the_kernel_lists(pqv, oracle):
    """Case 13: k * m = 1025 (host form: the range machinery and a host pass; device form: PQV_ERR_UNSUPPORTED), and 1100 probed lists."""
    st = Setup(pqv, oracle, 4096, 128, 8, seed=35)
    d = Grouped(pqv, st.s, st.n, st.rng.integers(0, st.n // 4, st.n).astype(np.int64))
    try:
        exp = d.check(st.queries[:2], 205, 5, st.kc, forms=("host",))
        assert (exp[4] == 205).all() and exp[3].max() > 1
        d.check(st.queries[:2], 204, 5, st.kc)              # (1020: the kernels)
        for k, m in ((205, 5), (1025, 1), (2 ** 31, 2)):    # (2^32 as a 32-bit product is 0)
            with pytest.raises(pqv.PqvError, match=UNSUPPORTED) as e:
                st.s.topk_grouped_device(8, 1, k, m, st.kc, d.keys, 8, 8)         # (refused before any pointer is read)
            assert e.value.code == -5
    finally:
        d.close()
    st = Setup(pqv, oracle, 2200, 8, 1100, seed=15)
    d = Grouped(pqv, st.s, st.n, st.rng.integers(0, st.n // 16, st.n).astype(np.int32), (st.rng.random(st.n) >= 0.3).astype(np.uint8))
    try:
        exp = d.check(st.queries[:2], 10, 3, 1100, forms=("host",))
        assert (exp[4] == 10).all()
        r, d2, g, c, nf, nc, _ = grouped_ref.grouped_topk(st.oidx.candidate_rows(st.queries[0], 1100), d.values, d.valid, None, st.data,
                                                          st.queries[0], 10, 3)
        assert (exp[0][0] == r).all() and (_bits(exp[1][0]) == _bits(d2)).all() and (exp[2][0] == g).all() and exp[5][0] == nc
        with pytest.raises(pqv.PqvError, match=UNSUPPORTED) as e:
            d.device(st.queries[:1], 10, 3, 1100)
        assert e.value.code == -5
    finally:
        d.close()


def test_second_submission_and_optional_outputs(pqv, oracle):
    """Case 14: the device outputs start as garbage (every call of _device), a second submission on the same lane buffers is
    bit-equal, and the optional outputs may be NULL."""
    import torch
    st = Setup(pqv, oracle, 1500, 30, 6, seed=19)
    d = Grouped(pqv, st.s, st.n, st.rng.integers(0, st.n // 16, st.n).astype(np.int64), (st.rng.random(st.n) >= 0.3).astype(np.uint8))
    try:
        a = d.device(st.queries, 13, 5, 3)
        d.device(st.queries, 128, 8, 2)                     # (other shapes through the same scratch in between)
        b = d.device(st.queries, 13, 5, 3)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
        dev = torch.device("cuda", 0)
        q_t = torch.from_numpy(st.queries).to(dev)
        nq = len(st.queries)
        r_t = torch.zeros((nq, 13, 5), dtype=torch.int32, device=dev); d_t = torch.zeros((nq, 13, 5), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        st.s.topk_grouped_device(q_t.data_ptr(), nq, 13, 5, 3, d.keys, r_t.data_ptr(), d_t.data_ptr(), sqrt_out=False)
        torch.cuda.synchronize()
        assert (r_t.cpu().numpy().view(np.uint32) == a[0]).all() and (_bits(d_t.cpu().numpy()) == _bits(a[1])).all()
        # sqrt_out: the IEEE square root of the same d2
        got = st.s.topk_grouped(st.queries, 13, 5, 3, d.keys)
        assert (got[0] == a[0]).all() and (_bits(got[1]) == _bits(np.sqrt(a[1]))).all()
        with pytest.raises(pqv.PqvError, match="group_size must be > 0"):
            st.s.topk_grouped(st.queries, 5, 0, 2, d.keys)
        with pytest.raises(pqv.PqvError, match="nprobe must be > 0"):
            st.s.topk_grouped(st.queries, 5, 2, 0, d.keys)
    finally:
        d.close()


@pytest.fixture(scope="module")
def small(pqv, oracle):
    """Case 14's set-up (1500 x 30, 6 lists), for the two tests below."""
    st = Setup(pqv, oracle, 1500, 30, 6, seed=19)
    d = Grouped(pqv, st.s, st.n, st.rng.integers(0, st.n // 16, st.n).astype(np.int64), (st.rng.random(st.n) >= 0.3).astype(np.uint8))
    yield st, d
    d.close()


def _outputs_alone(call, nq, k, m, full, given):
    """call(r, d, g, c, nf) with fresh garbage blocks, 0 in place of every optional output that `given` does not name; what it writes
    must equal, byte for byte, the same outputs of the all-outputs call `full` (_device's tuple), and the withheld ones are not missed."""
    import torch
    dev = torch.device("cuda", 0)
    r_t = torch.full((nq, k, m), 5, dtype=torch.int32, device=dev)
    d_t = torch.full((nq, k, m), -1.0, dtype=torch.float32, device=dev)
    opt = {"group_key": (torch.full((nq, k), 77, dtype=torch.int64, device=dev), 2),
           "group_rows": (torch.full((nq, k), 99, dtype=torch.int32, device=dev), 3),
           "n_found": (torch.full((nq,), 9, dtype=torch.int32, device=dev), 4)}
    torch.cuda.synchronize()
    call(r_t.data_ptr(), d_t.data_ptr(), *(opt[name][0].data_ptr() if name in given else 0 for name in ("group_key", "group_rows", "n_found")))
    torch.cuda.synchronize()
    what = f"m={m} given={given}"
    assert r_t.cpu().numpy().tobytes() == full[0].tobytes(), "rows " + what
    assert d_t.cpu().numpy().tobytes() == full[1].tobytes(), "distances " + what
    for name in given:
        t, i = opt[name]
        assert t.cpu().numpy().tobytes() == full[i].tobytes(), name + " " + what


@pytest.mark.parametrize("m", [1, 5])
def test_each_optional_output_alone(small, m):
    """The lane stands in for the group keys and n_found that a caller does not take but the fold reads (group keys: pass 2's
    set; n_found: the set and the rows-per-group fill): each of d_group_key, d_group_rows and d_n_found given alone."""
    st, d = small
    nq, k, nprobe = len(st.queries), 13, 3
    full = d.device(st.queries, k, m, nprobe)
    import torch
    q_t = torch.from_numpy(st.queries).to(torch.device("cuda", 0))
    for name in ("group_key", "group_rows", "n_found"):
        _outputs_alone(lambda r, dd, g, c, nf: st.s.topk_grouped_device(q_t.data_ptr(), nq, k, m, nprobe, d.keys, r, dd, g, c, nf,
                                                                        mask=d.shared_mask, sqrt_out=False),
                       nq, k, m, full, (name,))


def test_distinct_device_without_group_key_or_n_found(small):
    """topk_distinct_device with d_group_key = 0, and again with d_n_found = 0: the other outputs equal the all-outputs call's."""
    st, d = small
    nq, k, nprobe = len(st.queries), 13, 3
    import torch
    dev = torch.device("cuda", 0)
    q_t = torch.from_numpy(st.queries).to(dev)
    r_t = torch.full((nq, k, 1), 5, dtype=torch.int32, device=dev); d_t = torch.full((nq, k, 1), -1.0, dtype=torch.float32, device=dev)
    g_t = torch.full((nq, k), 77, dtype=torch.int64, device=dev); nf_t = torch.full((nq,), 9, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    st.s.topk_distinct_device(q_t.data_ptr(), nq, k, nprobe, d.keys, r_t.data_ptr(), d_t.data_ptr(), g_t.data_ptr(), nf_t.data_ptr(),
                              mask=d.shared_mask, sqrt_out=False)
    torch.cuda.synchronize()
    full = (r_t.cpu().numpy(), d_t.cpu().numpy(), g_t.cpu().numpy(), None, nf_t.cpu().numpy())
    assert (full[4] > 0).any() and (full[0] != 5).any()                     # (the call wrote something to compare with)
    for given in (("n_found",), ("group_key",)):
        _outputs_alone(lambda r, dd, g, c, nf: st.s.topk_distinct_device(q_t.data_ptr(), nq, k, nprobe, d.keys, r, dd, g, nf,
                                                                         mask=d.shared_mask, sqrt_out=False),
                       nq, k, 1, full, given)


def test_builders(pqv, tmp_path):
    """Case 15: .distinct_on("doc").group_size(3) on a written Parquet file with an int64 doc column, with and without .where(),
    and on a two-file table; against the yardstick on the same resident searcher."""
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

    def expect(s, column, allowed, k, m, nprobe):
        mk = s.row_mask(allowed)
        try:
            _, rows, dist, _, _ = s.range_search(query, np.inf, nprobe, mask=mk)
        finally:
            mk.close()
        return grouped_ref.group_sorted(rows, dist, column, k, m)

    s = pqv.searcher_for_parquet(paths[0])
    for where in (False, True):
        b = pqv.TopkBuilder(paths[0], query).k(7).nprobe(3).distinct_on("doc").group_size(3)
        if where:
            b = b.where(pqv.col("id") >= 2)
        res = b.search()
        r, dd, g, c, nf = expect(s, docs[0], np.arange(300) >= (2 if where else 0), 7, 3, 3)
        assert len(res) == nf == 7 and isinstance(res[0], pqv.GroupSearchResult) and isinstance(res[0].hits[0], pqv.SearchResult)
        assert [x.key for x in res] == g.tolist() and [len(x.hits) for x in res] == c.tolist() and max(c) > 1
        for i, x in enumerate(res):
            assert [h.row_idx for h in x.hits] == r[i, :c[i]].tolist()
            assert [np.float32(h.distance) for h in x.hits] == dd[i, :c[i]].tolist()
    # the table
    ts = pqv.searcher_for_parquet_files(paths)
    doc_all = np.concatenate(docs)
    for where in (False, True):
        b = pqv.TableTopkBuilder(paths, query).k(9).nprobe(2).distinct_on("doc").group_size(2)
        if where:
            b = b.where(pqv.col("id") >= 2)
        res = b.search()
        allowed = np.concatenate([np.arange(300) >= 2, np.arange(200) >= 2]) if where else np.ones(500, bool)
        r, dd, g, c, nf = expect(ts, doc_all, allowed, 9, 2, 2)
        assert len(res) == nf == 9 and [x.key for x in res] == g.tolist() and [len(x.hits) for x in res] == c.tolist()
        for i, x in enumerate(res):
            f, local = ts.split_rows(r[i, :c[i]])
            assert [h.path for h in x.hits] == [paths[int(j)] for j in f] and [h.row_idx for h in x.hits] == local.tolist()
            assert [np.float32(h.distance) for h in x.hits] == dd[i, :c[i]].tolist()
    with pytest.raises(pqv.PqvError, match=r"group_size\(\) needs distinct_on\(\)"):
        pqv.TopkBuilder(s, query).k(3).nprobe(1).group_size(2).search()


@pytest.mark.parametrize("filt", [None, "eq", "range", "in"])
def test_host_sub_batches(pqv, oracle, filt):
    """One host call of more queries than one sub-batch holds (k = 300, m = 3, 4096 x 128, all 8 lists): rows and distances land at
    q0 * k * m, group keys and group_rows at q0 * k, and the second sub-batch's filter slice is its own."""
    from test_gpu_distinct import check_host_sub_batches
    check_host_sub_batches(pqv, oracle, 3, filt)
