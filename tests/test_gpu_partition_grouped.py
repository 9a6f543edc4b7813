"""Distinct / grouped top-k over a key partition on the GPU (pqv_topk_partition_grouped, pqv_topk_partition_grouped_device).

Every call is compared, bit for bit, against the numpy restatement (tests/partition_group_ref.py over
tests/partition_group_cases.py) AND against pqv_topk_grouped_filtered_device on S1 -- a searcher over Index.from_parts(dim, one
centroid, [all indexed rows ascending]) on the same corpus, nprobe = 1, max_candidates = 0, row keys made from the same two columns
-- per the contract's equivalence, n_candidates excepted.  The inputs have no two rows equally far from a query (partition_cases),
so RANGE and IN qualify for the S1 comparison too; the one case with deliberate ties is held to the restatement's (distance,
position) order.  There are no tolerances."""
import ctypes as C

import numpy as np
import pytest

import key_filter_ref as kf
import long_rows_cases as lrc
import partition_cases as pc
import partition_group_cases as pgc
import partition_group_ref as pgr
import partition_ref as pr
from test_gpu_partition import Setup, _dev, _device_filter, _host_filter, _same, one_list, part_device

pytestmark = pytest.mark.gpu

EMPTY = 0xFFFFFFFF
DOT_TEXT = "PQV_DOT is not supported by keyed and distinct calls"
LIMIT_TEXT = "pqv_topk_partition_grouped takes k \\* group_size <= 1024"


def _outputs(nq, k, m):
    """rows, dist [nq, k, m], group_key, group_rows [nq, k], n_found, n_candidates [nq], filled with what no call writes"""
    import torch
    dev = _dev()
    return (torch.full((nq, k, m), 7, dtype=torch.int32, device=dev), torch.full((nq, k, m), -1.0, dtype=torch.float32, device=dev),
            torch.full((nq, k), 7, dtype=torch.int64, device=dev), torch.full((nq, k), 7, dtype=torch.int32, device=dev),
            torch.full((nq,), 7, dtype=torch.int32, device=dev), torch.full((nq,), 7, dtype=torch.int64, device=dev))


def _slot0(x):
    """the [.., 0] slots of a [nq, k, m] output, as an array of their own"""
    return np.ascontiguousarray(x[:, :, 0])


def _results(r_t, d_t, g_t, c_t, nf_t, nc_t):
    return (r_t.cpu().numpy().view(np.uint32), d_t.cpu().numpy(), g_t.cpu().numpy(), c_t.cpu().numpy().view(np.uint32),
            nf_t.cpu().numpy().view(np.uint32), nc_t.cpu().numpy().view(np.uint64))


def grouped_device(s, part, keys, q, k, m, flt, mask=None, metric=0, sqrt_out=False):
    """topk_partition_grouped_device -> (rows, dist, group_key, group_rows, n_found, n_candidates)"""
    import torch
    q_t = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(_dev())
    out = _outputs(len(q), k, m)
    kw, alive = _device_filter(flt)
    torch.cuda.synchronize()
    s.topk_partition_grouped_device(q_t.data_ptr(), len(q), k, m, part, keys, *[t.data_ptr() for t in out], mask=mask, metric=metric,
                                    sqrt_out=sqrt_out, **kw)
    torch.cuda.synchronize()
    del alive
    return _results(*out)


def s1_grouped(s1, fkeys1, gkeys1, q, k, m, flt, mask=None, metric=0, sqrt_out=False):
    """topk_grouped_device(filter_keys=...) on S1 with nprobe = 1 -> (rows, dist, group_key, group_rows, n_found)"""
    import torch
    q_t = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(_dev())
    out = _outputs(len(q), k, m)
    kw, alive = _device_filter(flt)
    torch.cuda.synchronize()
    s1.topk_grouped_device(q_t.data_ptr(), len(q), k, m, 1, gkeys1, *[t.data_ptr() for t in out], mask=mask, metric=metric,
                           sqrt_out=sqrt_out, filter_keys=fkeys1, **kw)
    torch.cuda.synchronize()
    del alive
    return _results(*out)[:5]


class GroupSetup(Setup):
    """test_gpu_partition.Setup plus, per group column, the searcher's row keys, S1's, and the grouped restatement"""

    def __init__(self, pqv, oracle, name, nq=5, flags=0, removed=None):
        super().__init__(pqv, oracle, name, nq, flags, removed)
        self.case = pgc.GroupCase(name, nq)
        self.gkeys, self.gkeys1 = {}, {}
        for gcol, (values, valid) in self.case.groups.items():
            col = pqv.Column.upload(values, valid)
            self.gkeys[gcol], self.gkeys1[gcol] = self.s.row_keys(col), self.s1.row_keys(col)
            col.close()

    def check(self, col, gcol, flt, k, m, allow=None, mask=None, mask1=None, sqrt_out=False, blocks=(0,), what=""):
        """the device form under every `blocks` == the restatement == the grouped filtered call on S1 -> (got, the restatement)"""
        c = self.case
        exp = c.grouped(self.ref[col], flt, gcol, k, m, sqrt_out=sqrt_out, allow=allow)
        for b in blocks:
            self.s.set_option("partition_blocks", b)
            got = grouped_device(self.s, self.parts[col], self.gkeys[gcol], c.queries, k, m, flt, mask=mask, metric=c.metric, sqrt_out=sqrt_out)
            _same(got, exp[:6], f"{what} {col} {gcol} {flt[0]} k={k} m={m} blocks={b} vs the restatement")
        self.s.set_option("partition_blocks", 0)
        twin = s1_grouped(self.s1, self.keys1[col], self.gkeys1[gcol], c.queries, k, m, flt, mask=mask1, metric=c.metric, sqrt_out=sqrt_out)
        _same(got[:5], twin, f"{what} {col} {gcol} {flt[0]} k={k} m={m} vs the grouped filtered call on S1")
        return got, exp


@pytest.fixture(scope="module", params=list(pc.SHAPES))
def shape(request, pqv, oracle):
    return GroupSetup(pqv, oracle, request.param)


@pytest.mark.parametrize("gcol", ["doc32", "doc64"])
@pytest.mark.parametrize("col", ["t3", "t64", "distinct", "skew"])
def test_every_filter_k_group_size_and_block_count(shape, col, gcol):
    """EQ, RANGE and IN over every filter column at every (k, group_size) of the distinct and the grouped forms, partition_blocks
    in {1, 3, by rule}: list slots S = 1, 4, 16 in both passes."""
    st = shape
    for flt in st.case.filters(col):
        for k, m in pgc.DISTINCT_KM + pgc.GROUPED_KM:
            got, _ = st.check(col, gcol, flt, k, m, blocks=pc.BLOCKS)
            rows, dist, gkey, grows, nf, nc = got
            assert (nf <= np.minimum(k, nc)).all() and (grows <= m).all()
            for q in range(st.case.nq):
                assert (rows[q, nf[q]:] == EMPTY).all() and np.isposinf(dist[q, nf[q]:]).all()
                assert (gkey[q, nf[q]:] == 0).all() and (grows[q, nf[q]:] == 0).all() and (grows[q, :nf[q]] >= 1).all()


def test_few_groups_give_n_found_below_k(shape):
    st = shape
    full = ("range", kf.RANGE, [kf.INT64_MIN] * st.case.nq, [kf.INT64_MAX] * st.case.nq)
    for k, m in ((10, 1), (10, 3), (1, 1024)):
        got, _ = st.check("t3", "few", full, k, m, blocks=pc.BLOCKS)
        assert (got[4] == min(k, 5)).all() and (got[3][:, :min(k, 5)] >= min(m, 200)).all(), "5 groups of some hundred rows each"


def test_single_row_groups_equal_the_plain_partition_call(shape):
    """every group value distinct and valid: slot 0 holds pqv_topk_partition_device's rows, distances and n_found, group_rows is 1"""
    st, c = shape, shape.case
    for col in ("t3", "t64"):
        for flt in c.filters(col):
            for k, m in ((10, 1), (300, 1), (10, 3), (100, 10)):
                got, _ = st.check(col, "single", flt, k, m)
                plain = part_device(st.s, st.parts[col], c.queries, k, flt, metric=c.metric)
                _same((_slot0(got[0]), _slot0(got[1]), got[4], got[5]), plain, f"{col} {flt[0]} k={k} m={m} vs pqv_topk_partition_device")
                assert (got[0][:, :, 1:] == EMPTY).all()
                for q in range(c.nq):
                    assert (got[3][q, :got[4][q]] == 1).all()


def test_group_size_one_host_form_and_distinct_wrapper(shape):
    """group_size 1 against m: the [.., 0] slots, group keys and n_found agree; the host form equals the device form;
    topk_partition_distinct is the m = 1 call"""
    st, c = shape, shape.case
    for col, gcol in (("t64", "doc32"), ("skew", "doc64")):
        for flt in c.filters(col):
            for (k, m), sqrt_out in (((10, 3), True), ((100, 10), False)):
                one = grouped_device(st.s, st.parts[col], st.gkeys[gcol], c.queries, k, 1, flt, metric=c.metric, sqrt_out=sqrt_out)
                many = grouped_device(st.s, st.parts[col], st.gkeys[gcol], c.queries, k, m, flt, metric=c.metric, sqrt_out=sqrt_out)
                _same((_slot0(many[0]), _slot0(many[1]), many[2], many[4], many[5]), (_slot0(one[0]), _slot0(one[1]), one[2], one[4], one[5]),
                      f"{col} {gcol} {flt[0]} k={k}: group_size 1 vs {m}")
                for mm, dev in ((1, one), (m, many)):
                    host = st.s.topk_partition_grouped(c.queries, k, mm, st.parts[col], st.gkeys[gcol], metric=c.metric, sqrt_out=sqrt_out,
                                                       **_host_filter(flt))
                    _same(host, dev, f"{col} {gcol} {flt[0]} k={k} m={mm}: host form")
                    _same(host, c.grouped(st.ref[col], flt, gcol, k, mm, sqrt_out=sqrt_out)[:6], f"{col} {gcol} {flt[0]} k={k} m={mm}: host vs restatement")
                d = st.s.topk_partition_distinct(c.queries, k, st.parts[col], st.gkeys[gcol], metric=c.metric, sqrt_out=sqrt_out, **_host_filter(flt))
                _same(d, (_slot0(one[0]), _slot0(one[1]), one[2], one[4], one[5]), "topk_partition_distinct")


def test_shared_mask_and_counters(shape):
    """about half the rows; a mask that empties whole groups; a mask that allows nothing; a mask together with doc64's NULLs.
    Excluded rows do not count; embeddings_fetched advances by the considered rows plus pass 2's; the same call twice returns the
    same bytes."""
    st, c = shape, shape.case
    doc32 = c.groups["doc32"][0]
    masks = ((np.random.default_rng(3).random(c.n) < 0.5, "doc32"), (doc32 % 3 != 0, "doc32"), (np.zeros(c.n, bool), "doc32"),
             (np.random.default_rng(4).random(c.n) < 0.5, "doc64"))
    for allow, gcol in masks:
        m_, m1 = st.s.row_mask(allow), st.s1.row_mask(allow)
        try:
            for col in ("t3", "distinct"):
                for flt in c.filters(col):
                    for k, m in ((10, 1), (10, 3), (512, 2)):
                        before = st.s.counters()
                        got, exp = st.check(col, gcol, flt, k, m, allow=allow, mask=m_, mask1=m1, what="masked")
                        after = st.s.counters()
                        assert after["queries"] - before["queries"] == c.nq
                        assert after["candidate_rows"] - before["candidate_rows"] == int(exp[5].sum())
                        assert after["embeddings_fetched"] - before["embeddings_fetched"] == exp[6] + (exp[7] if m > 1 else 0)
                        assert after["screened_pairs"] == before["screened_pairs"] and after["screen_survivors"] == before["screen_survivors"]
                        _same(got[5:], c.grouped(st.ref[col], flt, gcol, k, m)[5:6], "n_candidates is taken before the mask")
                        got_rows = got[0][got[0] != EMPTY]
                        assert allow[got_rows].all(), "an excluded row came back"
                        if not allow.any():
                            assert (got[4] == 0).all()
                        if gcol == "doc32" and allow is masks[1][0]:
                            assert (got[2][got[3] > 0] % 3 != 0).all(), "a group the mask empties came back"
            flt = c.filters("t3")[1]
            a = grouped_device(st.s, st.parts["t3"], st.gkeys[gcol], c.queries, 10, 3, flt, mask=m_, metric=c.metric)
            b = grouped_device(st.s, st.parts["t3"], st.gkeys[gcol], c.queries, 10, 3, flt, mask=m_, metric=c.metric)
            _same(a, b, "the same call twice")
            before = st.s.counters()
            host = st.s.topk_partition_grouped(c.queries, 10, 3, st.parts["t3"], st.gkeys[gcol], mask=m_, metric=c.metric, sqrt_out=False,
                                               **_host_filter(flt))
            after = st.s.counters()
            exp = c.grouped(st.ref["t3"], flt, gcol, 10, 3, allow=allow)
            _same(host, a, "host form under a mask")
            assert after["queries"] - before["queries"] == c.nq and after["candidate_rows"] - before["candidate_rows"] == int(exp[5].sum())
            assert after["embeddings_fetched"] - before["embeddings_fetched"] == exp[6] + exp[7]
        finally:
            m_.close()
            m1.close()


@pytest.mark.parametrize("name,layout", [("4096x128", "row"), ("1500x30", "release"), ("2048x32-seq", "row")])
def test_layouts(pqv, oracle, name, layout):
    flags = pqv.PQV_LAYOUT_ROW_ORDER if layout == "row" else pqv.PQV_RELEASE_ROW_ORDER
    st = GroupSetup(pqv, oracle, name, flags=flags)
    for col, gcol in (("t3", "doc64"), ("skew", "doc32")):
        for flt in st.case.filters(col):
            for k, m in ((10, 1), (300, 1), (10, 3), (64, 4)):
                st.check(col, gcol, flt, k, m, what=layout)


@pytest.mark.parametrize("name", ["4096x128", "1500x30"])
def test_removed_rows_are_absent(pqv, oracle, name):
    n = pc.SHAPES[name]["n"]
    removed = np.unique(np.random.default_rng(8).integers(0, n, n // 5))
    st = GroupSetup(pqv, oracle, name, removed=removed)
    for col, gcol in (("t3", "doc32"), ("t64", "doc64"), ("distinct", "doc32")):
        for flt in st.case.filters(col):
            for k, m in ((100, 1), (100, 10)):
                got, _ = st.check(col, gcol, flt, k, m, blocks=(1, 0), what="removed")
                assert not np.isin(got[0][got[0] != EMPTY], removed).any()


@pytest.mark.parametrize("name", ["768", "132-cos", "260", "134-dot"])
def test_long_rows_cosine_and_dot(pqv, oracle, name):
    """multi-chunk rows, zero-padded storage ("260"), PQV_COSINE through the cosine layout (normalised, halved); PQV_DOT is refused
    with the existing text in both forms"""
    lc = lrc.Case(name, oracle)
    metric = {"l2": lc.metric, "cos": pqv.PQV_COSINE, "dot": pqv.PQV_DOT}[lc.kind]
    corpus = pqv.Corpus.upload(lc.data)
    s = pqv.Searcher(pqv.Index.from_parts(lc.dim, lc.centroids, lc.lists), corpus)
    s1 = one_list(pqv, lc.dim, corpus, np.arange(lc.n))
    fcol, gcol = pqv.Column.upload(lc.tenant, lc.tenant_valid), pqv.Column.upload(lc.group, lc.group_valid)
    part, gkeys, fkeys1, gkeys1 = s.key_partition(fcol), s.row_keys(gcol), s1.row_keys(fcol), s1.row_keys(gcol)
    lims, vals = kf.sets_to_csr(lrc.QUERY_SETS)
    flts = [("eq", kf.EQ, list(lrc.QUERY_KEYS), None), ("range", kf.RANGE, list(lrc.QUERY_RANGES[0]), list(lrc.QUERY_RANGES[1])),
            ("in", kf.IN, [int(x) for x in lims], [int(x) for x in vals])]
    if lc.kind == "dot":
        for m in (1, 3):
            with pytest.raises(pqv.PqvError, match=DOT_TEXT) as e:
                s.topk_partition_grouped(lc.queries, 10, m, part, gkeys, metric=metric, **_host_filter(flts[0]))
            assert e.value.code == pqv._ffi.PQV_ERR_UNSUPPORTED
            with pytest.raises(pqv.PqvError, match=DOT_TEXT) as e:
                grouped_device(s, part, gkeys, lc.queries, 10, m, flts[0], metric=metric)
            assert e.value.code == pqv._ffi.PQV_ERR_UNSUPPORTED
        return
    d = pr.distances(lc.kind, lc.metric, lc.data, lc.queries)
    prows, pkeys = pr.build(lc.tenant, lc.tenant_valid, np.arange(lc.n))
    shared = lc.masks["1/2"]
    m_, m1 = s.row_mask(shared), s1.row_mask(shared)
    for flt in flts:
        for (k, m), sqrt_out in (((10, 1), True), ((300, 1), False), ((10, 3), True), ((64, 4), False)):
            for allow, mask, mask1 in ((None, None, None), (shared, m_, m1)):
                exp = pgr.grouped_batch(prows, pkeys, flt[1], flt[2], flt[3], d, lc.group, lc.group_valid, k, m, lc.kind, sqrt_out, allow)
                for b in pc.BLOCKS:
                    s.set_option("partition_blocks", b)
                    got = grouped_device(s, part, gkeys, lc.queries, k, m, flt, mask=mask, metric=metric, sqrt_out=sqrt_out)
                    _same(got, exp[:6], f"{name} {flt[0]} k={k} m={m} blocks={b}")
                s.set_option("partition_blocks", 0)
                host = s.topk_partition_grouped(lc.queries, k, m, part, gkeys, mask=mask, metric=metric, sqrt_out=sqrt_out, **_host_filter(flt))
                _same(host, got, f"{name} {flt[0]} k={k} m={m} host form")
                twin = s1_grouped(s1, fkeys1, gkeys1, lc.queries, k, m, flt, mask=mask1, metric=metric, sqrt_out=sqrt_out)
                _same(got[:5], twin, f"{name} {flt[0]} k={k} m={m} vs the grouped filtered call on S1")
    m_.close()
    m1.close()


def test_ties_follow_distance_then_position(pqv):
    data, queries, keys = pc.tie_case()
    groups = pgc.tie_groups()
    corpus = pqv.Corpus.upload(data)
    n, dim = data.shape
    lists = [np.arange(i, n, 3, dtype=np.uint32) for i in range(3)]
    s = pqv.Searcher(pqv.Index.from_parts(dim, np.zeros((3, dim), np.float32), lists), corpus)
    part = s.key_partition(pqv.Column.upload(keys))
    gkeys = s.row_keys(pqv.Column.upload(groups))
    prows, pkeys = pr.build(keys, None, np.arange(n))
    d = pr.distances("l2", pr.REF4, data, queries)
    lims, vals = kf.sets_to_csr([[0, 3], [1], [0, 1, 2, 3], [2, 9], []])
    for flt in (("eq", kf.EQ, [0, 1, 2, 3, 7], None), ("range", kf.RANGE, [0, 1, 0, 3, 2], [1, 3, 3, 3, 1]),
                ("in", kf.IN, [int(x) for x in lims], [int(x) for x in vals])):
        for k, m in ((1, 1), (7, 1), (3, 5), (7, 100)):
            exp = pgr.grouped_batch(prows, pkeys, flt[1], flt[2], flt[3], d, groups, None, k, m, "l2", True)
            for b in pc.BLOCKS:
                s.set_option("partition_blocks", b)
                _same(grouped_device(s, part, gkeys, queries, k, m, flt, sqrt_out=True), exp[:6], f"ties {flt[0]} k={k} m={m} blocks={b}")
            s.set_option("partition_blocks", 0)
            _same(s.topk_partition_grouped(queries, k, m, part, gkeys, **_host_filter(flt)), exp[:6], f"ties {flt[0]} k={k} m={m} host")


def test_piece_boundary(pqv):
    """one call of PARTITION_GRID_Q + 5 queries (32768: the grid's y, restated from csrc/api.cpp) on the smallest rows: 5 distinct
    queries and filters, tiled, so the reference is computed for 5 and tiled; every output array is checked past the boundary"""
    piece, n, dim, k, m = 32768, 300, 8, 3, 2
    nq = piece + 5
    rng = np.random.default_rng(77)
    data, q5 = rng.random((n, dim), dtype=np.float32), rng.random((5, dim), dtype=np.float32)
    tenant = rng.integers(0, 3, n).astype(np.int32)
    groups, gvalid = rng.integers(-20, 20, n).astype(np.int64), (rng.random(n) >= 0.1).astype(np.uint8)
    corpus = pqv.Corpus.upload(data)
    lists = [np.arange(i, n, 2, dtype=np.uint32) for i in range(2)]
    s = pqv.Searcher(pqv.Index.from_parts(dim, np.zeros((2, dim), np.float32), lists), corpus)
    part, gkeys = s.key_partition(pqv.Column.upload(tenant)), s.row_keys(pqv.Column.upload(groups, gvalid))
    prows, pkeys = pr.build(tenant, None, np.arange(n))
    d5 = pr.distances("l2", pr.REF4, data, q5)
    reps = (nq + 4) // 5
    tile = lambda x: np.concatenate([x] * reps)[:nq]        # noqa: E731
    queries = tile(q5)
    sets5 = [[0], [1, 2], [], [0, 2, 5], [2]]
    lims5, vals5 = kf.sets_to_csr(sets5)
    lims, vals = kf.sets_to_csr((sets5 * reps)[:nq])
    for f5, f in ((("eq", kf.EQ, [0, 1, 2, 7, 1], None), ("eq", kf.EQ, ([0, 1, 2, 7, 1] * reps)[:nq], None)),
                  (("range", kf.RANGE, [0, 1, 2, 0, 1], [1, 2, 0, 2, 1]), ("range", kf.RANGE, ([0, 1, 2, 0, 1] * reps)[:nq], ([1, 2, 0, 2, 1] * reps)[:nq])),
                  (("in", kf.IN, [int(x) for x in lims5], [int(x) for x in vals5]), ("in", kf.IN, [int(x) for x in lims], [int(x) for x in vals]))):
        exp5 = pgr.grouped_batch(prows, pkeys, f5[1], f5[2], f5[3], d5, groups, gvalid, k, m, "l2", False)
        exp = [tile(x) for x in exp5[:6]]
        assert exp[4][piece:].max() > 0
        got = grouped_device(s, part, gkeys, queries, k, m, f)
        _same(got, exp, f"{f[0]}: {nq} queries in one device call")
        _same([x[piece:] for x in got], [x[piece:] for x in exp], f"{f[0]}: past the piece boundary")
    host = s.topk_partition_grouped(queries, k, m, part, gkeys, sqrt_out=False, **_host_filter(f))
    _same(host, exp, "the host form's sub-batches")


def test_device_filter_arrays_written_on_the_call_stream(shape):
    """the descriptor's device arrays are read inside the enqueued work: written on the same stream just before the call, with no
    synchronisation in between"""
    import torch
    st, c = shape, shape.case
    stream = torch.cuda.Stream()
    for flt in c.filters("t64"):
        exp = c.grouped(st.ref["t64"], flt, "doc64", 10, 3)
        a_host = torch.tensor([int(x) for x in flt[2]], dtype=torch.int64).pin_memory()
        b_host = torch.tensor([int(x) for x in (flt[3] or [0])] or [0], dtype=torch.int64).pin_memory()
        q_host = torch.from_numpy(c.queries).pin_memory()
        out = _outputs(c.nq, 10, 3)
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
            st.s.topk_partition_grouped_device(q_t.data_ptr(), c.nq, 10, 3, st.parts["t64"], st.gkeys["doc64"], *[t.data_ptr() for t in out],
                                               metric=c.metric, sqrt_out=False, stream=stream.cuda_stream, **kw)
        stream.synchronize()
        _same(_results(*out), exp[:6], f"{flt[0]} on a caller's stream")


def test_refusals_limits_and_lifetimes(pqv, oracle):
    import torch
    c = pgc.GroupCase("1500x30", nq=5)
    built = oracle.build_index(c.data, n_clusters=c.kc, max_iters=5, workers=1)
    lists = [np.asarray(l, np.uint32) for l in built.lists()]
    corpus = pqv.Corpus.upload(c.data)
    index = pqv.Index.from_parts(c.dim, built.centroids, lists)
    fcol, gcol = pqv.Column.upload(*c.columns["t64"]), pqv.Column.upload(*c.groups["doc64"])
    flt = c.filters("t64")[0]
    ref = c.partition("t64")
    exp = c.grouped(ref, flt, "doc64", 10, 3)
    s, other = pqv.Searcher(index, corpus), pqv.Searcher(index, corpus)
    p, keys = s.key_partition(fcol), s.row_keys(gcol)
    op, okeys, om = other.key_partition(fcol), other.row_keys(gcol), other.row_mask(np.ones(c.n, bool))
    host = lambda k=10, m=3, part=p, kk=keys, mask=None, metric=c.metric, q=c.queries: s.topk_partition_grouped(       # noqa: E731
        q, k, m, part, kk, mask=mask, metric=metric, query_keys=flt[2])
    dev = lambda k=10, m=3, part=p, kk=keys, mask=None, metric=c.metric, q=c.queries: grouped_device(                  # noqa: E731
        s, part, kk, q, k, m, flt, mask=mask, metric=metric)
    for call in (host, dev):
        # the error texts, in order: a partition, row keys and a mask of another searcher
        with pytest.raises(pqv.PqvError, match="key partition belongs to another searcher"):
            call(part=op, kk=okeys, mask=om)
        with pytest.raises(pqv.PqvError, match="row keys belong to another searcher"):
            call(kk=okeys, mask=om)
        with pytest.raises(pqv.PqvError, match="row mask belongs to another searcher"):
            call(mask=om)
        with pytest.raises(pqv.PqvError, match="k must be > 0"):
            call(k=0, m=0, part=op)
        with pytest.raises(pqv.PqvError, match="group_size must be > 0"):
            call(m=0, part=op)
        with pytest.raises(pqv.PqvError, match="unknown metric"):
            call(k=513, m=2, metric=9)
        # the two UNSUPPORTED texts behind everything else, PQV_DOT first; there is no host fallback
        with pytest.raises(pqv.PqvError, match=DOT_TEXT) as e:
            call(k=513, m=2, metric=pqv.PQV_DOT)
        assert e.value.code == pqv._ffi.PQV_ERR_UNSUPPORTED
        for k, m in ((513, 2), (1025, 1), (1, 1026)):
            with pytest.raises(pqv.PqvError, match=LIMIT_TEXT) as e:
                call(k=k, m=m)
            assert e.value.code == pqv._ffi.PQV_ERR_UNSUPPORTED
    with pytest.raises(pqv.PqvError, match="Query dimension mismatch: expected 30, got 29"):
        host(q=c.queries[:, :29], k=513, m=2)
    # 2^31 * 2^31: the product is taken in 64 bits (no output of that size exists: the raw entry points, which refuse before they touch one)
    lib, _ffi = pqv._ffi.lib(), pqv._ffi
    qk = (C.c_int64 * c.nq)(*flt[2])
    f = _ffi.KeyFilter(_ffi.PQV_KEY_EQ, 0, C.cast(qk, C.c_void_p), None)
    small_r, small_d = (C.c_uint32 * 8)(), (C.c_float * 8)()
    q = np.ascontiguousarray(c.queries)
    rc = lib.pqv_topk_partition_grouped(s._h, p._h, C.byref(f), keys._h, None, q.ctypes.data_as(C.POINTER(C.c_float)), c.nq, c.dim, 2 ** 31, 2 ** 31,
                                        0, 1, small_r, small_d, None, None, None, None)
    assert rc == _ffi.PQV_ERR_UNSUPPORTED and b"k * group_size <= 1024" in lib.pqv_last_error()
    t = torch.zeros(8, dtype=torch.int64, device=_dev())
    with pytest.raises(pqv.PqvError, match=LIMIT_TEXT):
        s.topk_partition_grouped_device(t.data_ptr(), c.nq, 2 ** 31, 2 ** 31, p, keys, t.data_ptr(), t.data_ptr(), query_keys=t.data_ptr())
    # nq = 0
    r0 = s.topk_partition_grouped(c.queries[:0], 10, 3, p, keys, query_keys=[])
    assert r0[0].shape == (0, 10, 3) and r0[2].shape == (0, 10)
    s.topk_partition_grouped_device(0, 0, 10, 3, p, keys, 0, 0, query_keys=0)
    # NULL optional outputs: rows and distances alone, for both forms of the call
    q_t = torch.from_numpy(c.queries).to(_dev())
    kw, alive = _device_filter(flt)
    for m in (1, 3):
        e = c.grouped(ref, flt, "doc64", 10, m)
        out = _outputs(c.nq, 10, m)
        torch.cuda.synchronize()
        s.topk_partition_grouped_device(q_t.data_ptr(), c.nq, 10, m, p, keys, out[0].data_ptr(), out[1].data_ptr(), metric=c.metric,
                                        sqrt_out=False, **kw)
        torch.cuda.synchronize()
        _same(_results(*out)[:2], e[:2], f"m={m}: rows and distances alone")
        assert (out[2] == 7).all() and (out[3] == 7).all() and (out[4] == 7).all() and (out[5] == 7).all()
        # ... and group_rows alone of the optional ones
        out = _outputs(c.nq, 10, m)
        s.topk_partition_grouped_device(q_t.data_ptr(), c.nq, 10, m, p, keys, out[0].data_ptr(), out[1].data_ptr(), 0, out[3].data_ptr(),
                                        metric=c.metric, sqrt_out=False, **kw)
        torch.cuda.synchronize()
        _same((_results(*out)[0], _results(*out)[1], _results(*out)[3]), (e[0], e[1], e[3]), f"m={m}: group_rows without n_found")
    del alive
    # the columns are not kept; partition, keys and searcher freed in any order after the call has completed
    fcol.close()
    gcol.close()
    _same(dev(), exp[:6])
    for order in ("pks", "kps", "skp"):
        s2 = pqv.Searcher(index, corpus)
        c1, c2 = pqv.Column.upload(*c.columns["t64"]), pqv.Column.upload(*c.groups["doc64"])
        h = {"p": s2.key_partition(c1), "k": s2.row_keys(c2), "s": s2}
        _same(grouped_device(s2, h["p"], h["k"], c.queries, 10, 3, flt, metric=c.metric), exp[:6], order)
        for ch in order:
            h[ch].close()
    for x in (op, okeys, om, other, p, keys, s):
        x.close()
