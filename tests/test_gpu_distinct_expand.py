"""Expanding distinct / grouped top-k on the GPU (pqv_topk_distinct_expand*, pqv_topk_grouped_expand*; Searcher.topk_distinct /
topk_grouped(max_nprobe=) and their _device forms (max_nprobe=, d_nprobe_used=); TopkBuilder.distinct_on().max_nprobe()).

The yardstick is never the code under test.  nprobe_used comes from tests/distinct_expand_ref.py (numpy over the ORACLE's probe
order).  For each distinct expected value u ONE existing twin call (topk_distinct / topk_grouped without max_nprobe) runs on the
whole batch with nprobe = u, and the queries whose expected depth is u must equal it bit for bit: rows, distance bits, group keys,
group_rows, n_found and n_candidates.  Host form and device form; the device form runs on a stream of the caller's with its filter
arrays uploaded on that stream.

The main fixtures (tests/distinct_expand_cases.py) are checked for vacuity on the CPU by tests/test_distinct_expand_host.py; every
other test asserts its own premise on the REFERENCE's depths before it compares anything."""
import ctypes as C

import numpy as np
import pytest

import distinct_expand_cases as cases
import distinct_expand_ref as dref
import distinct_filter_ref as fref
import expand_ref
from distinct_filter_ref import EQ, IN, RANGE

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1
UNSUPPORTED = -5


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class St:
    """a searcher over the oracle's centroids and lists, a group column, an optional filter column and shared mask"""

    def __init__(self, pqv, oracle, data, oidx, lists, group, gvalid=None, fvalues=None, fvalid=None, shared=None, flags=0):
        self.pqv, self.oracle, self.oidx, self.lists, self.data = pqv, oracle, oidx, lists, data
        self.group, self.gvalid, self.fvalues, self.fvalid, self.shared = group, gvalid, fvalues, fvalid, shared
        self.corpus = pqv.Corpus.upload(data)
        self.s = pqv.Searcher(pqv.Index.from_parts(data.shape[1], oidx.centroids, lists), self.corpus, flags)
        col = pqv.Column.upload(group, None if gvalid is None else gvalid.astype(np.uint8), device=0)
        self.gkeys = self.s.row_keys(col)
        col.close()
        self.fkeys = None
        if fvalues is not None:
            col = pqv.Column.upload(fvalues, None if fvalid is None else fvalid.astype(np.uint8), device=0)
            self.fkeys = self.s.row_keys(col)
            col.close()
        self.mask = self.s.row_mask(shared) if shared is not None else None
        self.order_oidx, self.order_q = oidx, (lambda q: q)

    def close(self):
        for h in (self.mask, self.fkeys, self.gkeys, self.s):
            if h is not None:
                h.close()

    def M(self, kind, spec, nq):
        if kind is None:
            return self.shared
        return np.stack([fref.allowed(self.fvalues, self.fvalid, kind, spec, i, self.shared) for i in range(nq)])

    def model(self, q, kind, spec, k, nprobe, max_nprobe):
        return dref.used_for_batch(self.order_oidx, self.lists, self.group, self.gvalid, self.M(kind, spec, len(q)), self.order_q(q), k,
                                   nprobe, max_nprobe)

    def host(self, q, k, m, nprobe, kind=None, spec=None, max_nprobe=None, metric=0, sqrt_out=False):
        kw = dict(mask=self.mask, metric=metric, sqrt_out=sqrt_out, max_nprobe=max_nprobe)
        if kind is not None:
            kw.update(filter_keys=self.fkeys, **fref.call_kw(kind, spec))
        if m is None:
            return self.s.topk_distinct(q, k, nprobe, self.gkeys, **kw)
        return self.s.topk_grouped(q, k, m, nprobe, self.gkeys, **kw)

    def device(self, q, k, m, nprobe, kind=None, spec=None, max_nprobe=None, metric=0, sqrt_out=False, raw=False):
        """the device form on a stream of the caller's: the queries and the filter arrays are uploaded ON that stream, the outputs are
        pre-filled with garbage there, and one synchronise of the stream follows the call"""
        import torch
        dev = torch.device("cuda", 0)
        nq = len(q)
        side = torch.cuda.Stream(device=dev)
        shape = (nq, k) if m is None else (nq, k, m)
        with torch.cuda.stream(side):
            q_t = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(dev, non_blocking=True)
            fkw, alive = {}, ()
            if kind is not None:
                _, a, b = fref.descriptor(kind, spec)
                a_t = torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev, non_blocking=True)
                if kind == EQ:
                    fkw, alive = {"query_keys": a_t.data_ptr()}, (a_t,)
                else:
                    b_t = torch.from_numpy(np.ascontiguousarray(b if len(b) else np.zeros(1, np.int64))).to(dev, non_blocking=True)
                    fkw, alive = {"query_key_ranges" if kind == RANGE else "query_key_sets": (a_t.data_ptr(), b_t.data_ptr())}, (a_t, b_t)
                fkw["filter_keys"] = self.fkeys
            r_t = torch.full(shape, 5, dtype=torch.int32, device=dev)
            d_t = torch.full(shape, -1.0, dtype=torch.float32, device=dev)
            g_t = torch.full((nq, k), 77, dtype=torch.int64, device=dev)
            c_t = torch.full((nq, k), 99, dtype=torch.int32, device=dev)
            nf_t = torch.full((nq,), 9, dtype=torch.int32, device=dev)
            nc_t = torch.full((nq,), 9, dtype=torch.int64, device=dev)
            u_t = torch.full((nq,), 7777, dtype=torch.int32, device=dev)
            kw = dict(mask=self.mask, metric=metric, sqrt_out=sqrt_out, stream=side.cuda_stream, **fkw)
            if max_nprobe:
                kw.update(max_nprobe=max_nprobe, d_nprobe_used=u_t.data_ptr())
            if m is None:
                self.s.topk_distinct_device(q_t.data_ptr(), nq, k, nprobe, self.gkeys, r_t.data_ptr(), d_t.data_ptr(), g_t.data_ptr(),
                                            nf_t.data_ptr(), nc_t.data_ptr(), **kw)
            else:
                self.s.topk_grouped_device(q_t.data_ptr(), nq, k, m, nprobe, self.gkeys, r_t.data_ptr(), d_t.data_ptr(), g_t.data_ptr(),
                                           c_t.data_ptr(), nf_t.data_ptr(), nc_t.data_ptr(), **kw)
        side.synchronize()
        del alive
        out = [r_t.cpu().numpy().view(np.uint32), d_t.cpu().numpy(), g_t.cpu().numpy()]
        if m is not None:
            out.append(c_t.cpu().numpy().view(np.uint32))
        out += [nf_t.cpu().numpy().astype(np.uint32), nc_t.cpu().numpy().astype(np.uint64)]
        if max_nprobe:
            out.append(u_t.cpu().numpy().astype(np.uint32))
        return tuple(x.tobytes() for x in out) if raw else tuple(out)

    def check(self, q, k, m, nprobe, max_nprobe, kind=None, spec=None, metric=0, premise=None, forms=("host", "device"), what=""):
        """the module's yardstick for one expanding call -> (the model's nprobe_used, the first form's result)"""
        exp_used = self.model(q, kind, spec, k, nprobe, max_nprobe)
        what = f"{what} kind={kind} k={k} m={m} nprobe={nprobe} max={max_nprobe} expected used {exp_used.tolist()}"
        if premise:
            assert premise(exp_used), "premise missed: " + what
        names = ("rows", "distance bits", "group keys") + (() if m is None else ("group_rows",)) + ("n_found", "n_candidates")
        got = {f: getattr(self, f)(q, k, m, nprobe, kind, spec, max_nprobe=max_nprobe, metric=metric) for f in forms}
        for f in forms:
            assert len(got[f]) == len(names) + 1
            assert (got[f][-1] == exp_used).all(), f"{f} nprobe_used {got[f][-1].tolist()}: {what}"
        for u in sorted(set(exp_used.tolist())):
            sel = exp_used == u
            for f in forms:
                twin = getattr(self, f)(q, k, m, u, kind, spec, metric=metric)
                assert len(twin) == len(names)
                for name, x, y in zip(names, got[f], twin):
                    x, y = np.asarray(x)[sel], np.asarray(y)[sel]
                    assert x.shape == y.shape and (x.view(np.uint8) == y.view(np.uint8)).all(), f"{f} form against its twin at nprobe={u}: {name}: {what}"
        return exp_used, got[forms[0]]


def _main_st(pqv, oracle, name):
    c, b = cases.case(oracle, name), cases.base(oracle)
    return c, St(pqv, oracle, b["data"], b["built"], b["lists"], c["group"], gvalid=c["gvalid"], fvalues=c["fvalues"], shared=c["shared"])


@pytest.fixture(scope="module", params=list(cases.MAIN))
def main(request, pqv, oracle):
    c, st = _main_st(pqv, oracle, request.param)
    yield c, st
    st.close()


@pytest.fixture(scope="module")
def eq_case(pqv, oracle):
    c, st = _main_st(pqv, oracle, "eq")
    yield c, st
    st.close()


@pytest.fixture(scope="module")
def range_case(pqv, oracle):
    c, st = _main_st(pqv, oracle, "range")
    yield c, st
    st.close()


def test_forms_distinct(main):
    """unfiltered (a column with NULLs), under a shared mask, EQ, RANGE, IN: host and device form, at least three depths with p0 and P
    among them (tests/test_distinct_expand_host.py holds the fixture to that)"""
    c, st = main
    u, got = st.check(c["queries"], c["k"], None, c["nprobe"], c["max_nprobe"], c["kind"], c["spec"], premise=lambda u: (u == c["used"]).all(),
                      what=c["name"])
    nf = got[3]
    assert nf[0] == c["k"] and nf[1] == c["k"] - 1                # query A finds exactly k groups in its P lists, B one fewer
    if c["gvalid"] is not None:                                   # a NULL row is never returned
        rows = got[0][got[0] != 0xFFFFFFFF]
        assert c["gvalid"][rows].all()


def test_forms_grouped(main):
    c, st = main
    u, got = st.check(c["queries"], c["k"], 3, c["nprobe"], c["max_nprobe"], c["kind"], c["spec"], what=c["name"] + " grouped")
    assert got[4][0] == c["k"] and got[4][1] == c["k"] - 1 and (got[3] <= 3).all() and (got[3] > 1).any()


def test_optional_outputs_null_and_nq_zero(eq_case):
    c, st = eq_case
    import torch
    from pq_vector_amd import _ffi
    lib, q, k, nq = _ffi.lib(), c["queries"], c["k"], len(c["queries"])
    full = st.host(q, k, None, c["nprobe"], c["kind"], c["spec"], max_nprobe=c["max_nprobe"])
    rows, dist = np.zeros((nq, k), np.uint32), np.zeros((nq, k), np.float32)
    _, a, _b = fref.descriptor(c["kind"], c["spec"])
    f = _ffi.KeyFilter(_ffi.PQV_KEY_EQ, 0, a.ctypes.data, None)
    u32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    assert lib.pqv_topk_distinct_expand(st.s._h, st.gkeys._h, st.fkeys._h, C.byref(f), None, q.ctypes.data_as(f32p), nq, q.shape[1], k,
                                        c["nprobe"], c["max_nprobe"], 0, 0, rows.ctypes.data_as(u32p), dist.ctypes.data_as(f32p), None,
                                        None, None, None) == 0
    assert (rows == full[0]).all() and (_bits(dist) == _bits(full[1])).all()
    rows3, dist3 = np.zeros((nq, k, 3), np.uint32), np.zeros((nq, k, 3), np.float32)
    full3 = st.host(q, k, 3, c["nprobe"], c["kind"], c["spec"], max_nprobe=c["max_nprobe"])
    assert lib.pqv_topk_grouped_expand(st.s._h, st.gkeys._h, st.fkeys._h, C.byref(f), None, q.ctypes.data_as(f32p), nq, q.shape[1], k, 3,
                                       c["nprobe"], c["max_nprobe"], 0, 0, rows3.ctypes.data_as(u32p), dist3.ctypes.data_as(f32p), None,
                                       None, None, None, None) == 0
    assert (rows3 == full3[0]).all() and (_bits(dist3) == _bits(full3[1])).all()
    # the device forms with every optional output left out
    dev = torch.device("cuda", 0)
    q_t = torch.from_numpy(q).to(dev)
    a_t = torch.from_numpy(a).to(dev)
    r_t = torch.zeros((nq, k), dtype=torch.int32, device=dev)
    d_t = torch.zeros((nq, k), dtype=torch.float32, device=dev)
    r3_t = torch.zeros((nq, k, 3), dtype=torch.int32, device=dev)
    d3_t = torch.zeros((nq, k, 3), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    kw = dict(filter_keys=st.fkeys, query_keys=a_t.data_ptr(), max_nprobe=c["max_nprobe"], sqrt_out=False)
    st.s.topk_distinct_device(q_t.data_ptr(), nq, k, c["nprobe"], st.gkeys, r_t.data_ptr(), d_t.data_ptr(), **kw)
    st.s.topk_grouped_device(q_t.data_ptr(), nq, k, 3, c["nprobe"], st.gkeys, r3_t.data_ptr(), d3_t.data_ptr(), **kw)
    torch.cuda.synchronize()
    assert (r_t.cpu().numpy().view(np.uint32) == full[0]).all() and (_bits(d_t.cpu().numpy()) == _bits(full[1])).all()
    assert (r3_t.cpu().numpy().view(np.uint32) == full3[0]).all() and (_bits(d3_t.cpu().numpy()) == _bits(full3[1])).all()
    # nq == 0
    out = st.s.topk_distinct(np.zeros((0, q.shape[1]), np.float32), k, 1, st.gkeys, max_nprobe=4)
    assert len(out) == 6 and out[0].shape == (0, k) and out[5].shape == (0,)
    st.s.topk_grouped_device(0, 0, k, 3, 1, st.gkeys, 0, 0, max_nprobe=4)


@pytest.mark.parametrize("k", [1, 10, 64, 65, 300])
def test_list_widths_distinct(range_case, k):
    """S = 1 / 4 / 16 lists and the 64 / 65 edge, every list of the index within reach; a tenant range passes about 330 groups"""
    c, st = range_case
    premise = (lambda u: (u <= 2).all()) if k == 1 else (lambda u: len(set(u.tolist())) >= 3)
    u, got = st.check(c["queries"], k, None, 1, 64, c["kind"], c["spec"], premise=premise, what="widths")
    if k == 300:
        assert (u == 64).any() and (got[3] < 300).any()


@pytest.mark.parametrize("k,m", [(10, 3), (256, 4), (341, 3)])
def test_list_widths_grouped(range_case, k, m):
    c, st = range_case
    st.check(c["queries"][:8], k, m, 2, 64, c["kind"], (c["spec"][0][:8], c["spec"][1][:8]),
             premise=(lambda u: len(set(u.tolist())) >= 3) if k <= 256 else (lambda u: (u == 64).all()),
             forms=("device",) if k > 10 else ("host", "device"), what="grouped widths")


def _line_index(oracle, dim, lens):
    """centroids 10 apart on a line, list c holding lens[c] rows around centroid c: a query at 10 c + 1 probes c, c + 1, c - 1, ..."""
    kc = len(lens)
    cents = np.zeros((kc, dim), np.float32)
    cents[:, 0] = 10.0 * np.arange(kc)
    rng = np.random.default_rng(99)
    n = int(sum(lens))
    rows = rng.permutation(n).astype(np.uint32)
    lists, at = [], 0
    data = rng.random((n, dim), dtype=np.float32)
    for ci, ln in enumerate(lens):
        lists.append(np.sort(rows[at:at + ln]))
        data[lists[-1].astype(np.int64), 0] += 10.0 * ci
        at += ln
    return data, oracle.index_from_parts(dim, cents, lists), lists


def test_list_lengths_and_per_query_conditions(pqv, oracle):
    """lists of 0, 1, 63, 64, 65 and 1025 rows among the probed ones (dim 10: unaligned rows); a group seen at rank 0 and again at
    rank 5 counts once; a crossing before rank p0 - 1 still gives p0; an empty IN slice gives used == P and nothing found"""
    lens = [64, 0, 1, 63, 65, 1025, 7, 64, 130, 0, 33, 1]
    data, oidx, lists = _line_index(oracle, 10, lens)
    n = len(data)
    rng = np.random.default_rng(3)
    group = rng.integers(-50, 350, n).astype(np.int32)            # I32, negative values, about 4 rows per group
    # query 0 starts in list 0: all of list 0 is ONE group, which comes back in the list of its rank 5; the lists between hold 3 groups
    q = np.zeros((6, 10), np.float32)
    q[:, 0] = [1.0, 21.0, 49.0, 71.0, 52.0, 101.0]
    q[:, 1:] = 0.5
    order0 = expand_ref.probe_order(oidx, q[0], 12).tolist()
    assert order0[0] == 0 and all(len(lists[c]) in lens for c in order0)
    group[lists[0].astype(np.int64)] = 1000
    between = np.concatenate([lists[c] for c in order0[1:5]]).astype(np.int64)
    group[between] = 2000 + (np.arange(len(between)) % 3)
    group[lists[order0[5]].astype(np.int64)] = 1000
    tenant = rng.integers(0, 4, n).astype(np.int64)
    st = St(pqv, oracle, data, oidx, lists, group, fvalues=tenant)
    try:
        cnt0 = dref.gcnt(oidx, lists, group, None, None, q[0], 12)
        assert cnt0[:6].tolist() == [1, 1, 2, 4, 4, 4] or (cnt0[0] == 1 and cnt0[4] == 4 and cnt0[5] == 4), cnt0.tolist()
        u, _ = st.check(q, 5, None, 1, 12, premise=lambda u: u[0] > 6 and len(set(u.tolist())) >= 2, what="lengths")
        st.check(q, 5, 2, 1, 12, what="lengths grouped")
        st.check(q, 70, None, 2, 12, premise=lambda u: len(set(u.tolist())) >= 2, what="lengths k 70")
        # the crossing at rank 0, p0 = 3
        u, _ = st.check(q, 1, None, 3, 12, premise=lambda u: (u == 3).all(), what="p0 3")
        # per-query filters, an empty IN slice among them
        sets = [{0, 1}, set(), {2}, {3, 0}, {1}, {0, 1, 2, 3}]
        u, got = st.check(q, 5, None, 1, 12, IN, sets, premise=lambda u: u[1] == 12 and (u < 12).any(), what="IN with an empty slice")
        assert got[3][1] == 0 and (got[0][1] == 0xFFFFFFFF).all()
        st.check(q, 5, 2, 1, 12, EQ, [0, 1, 2, 3, 9, 0], premise=lambda u: u[4] == 12, what="EQ grouped")
    finally:
        st.close()


def test_group_columns(pqv, oracle, eq_case):
    """a column of ONE group (used == P for k > 1); a column with the set's empty marker, 0, -1 and both i64 extremes; a column whose
    values are equal modulo the set's size -- on the base index, unfiltered"""
    b = cases.base(oracle)
    q = b["pool"][:8]
    rng = np.random.default_rng(17)
    one = np.full(cases.N, I64_MIN, np.int64)
    special = np.array([-1, 0, I64_MIN, I64_MAX, 1, -2], np.int64)[rng.integers(0, 6, cases.N)]
    congruent = (7 + dref.SET_SLOTS * rng.integers(0, 1100, cases.N)).astype(np.int64)
    for name, group, k, P, premise in (("one group", one, 2, 8, lambda u: (u == 8).all()),
                                       ("one group k 1", one, 1, 8, lambda u: (u == 1).all()),
                                       ("special values", special, 6, 8, lambda u: (u < 8).all()),
                                       ("special values short", special, 7, 8, lambda u: (u == 8).all()),
                                       ("congruent", congruent, 300, 64, lambda u: len(set(u.tolist())) >= 2),
                                       ("congruent all", congruent, 1024, 64, None)):
        st = St(pqv, oracle, b["data"], b["built"], b["lists"], group)
        try:
            u, got = st.check(q, k, None, 1, P, premise=premise, forms=("device",) if k > 300 else ("host", "device"), what=name)
            if name == "special values":
                assert set(got[2][got[0] != 0xFFFFFFFF].tolist()) == set(special.tolist())
            if name == "special values short":
                assert (got[3] == 6).all()
        finally:
            st.close()


def test_layouts_metrics_clamps(pqv, oracle, main):
    """max_nprobe == nprobe is the twin; P clamps to n_clusters; both layouts; PQV_L2SQ_SEQ"""
    c, st = main
    q = c["queries"]
    st.check(q, c["k"], None, 3, 3, c["kind"], c["spec"], premise=lambda u: (u == 3).all(), what="max == nprobe")
    st.check(q, c["k"], None, c["nprobe"], 1000, c["kind"], c["spec"], premise=lambda u: (u <= 64).all() and (u > c["max_nprobe"]).any(),
             forms=("device",),
             what="max 1000")
    st.check(q, c["k"], None, c["nprobe"], c["max_nprobe"], c["kind"], c["spec"], metric=st.pqv.PQV_L2SQ_SEQ, forms=("device",), what="SEQ")
    b = cases.base(oracle)
    for flags in (st.pqv.PQV_LAYOUT_ROW_ORDER, st.pqv.PQV_LAYOUT_IVF_ORDERED):
        alt = St(st.pqv, oracle, b["data"], b["built"], b["lists"], c["group"], gvalid=c["gvalid"], fvalues=c["fvalues"], shared=c["shared"],
                 flags=flags)
        try:
            alt.check(q, c["k"], 3, c["nprobe"], c["max_nprobe"], c["kind"], c["spec"], forms=("host",), what=f"layout flags {flags}")
        finally:
            alt.close()


def test_mask_one_in_64_alone_and_with_a_filter(pqv, oracle):
    """the 1/64 mask alone, and the 1/8 mask under a tenant filter per query"""
    b = cases.base(oracle)
    q = b["pool"][16:32]
    lo = [i % cases.TENANTS for i in range(16)]
    spec = (lo, [min(t + 3, cases.TENANTS - 1) for t in lo])
    for shared, k, kind, sp in ((b["mask64"], 3, None, None), (b["mask8"], 5, RANGE, spec), (b["mask8"], 5, IN, [{t, (t + 4) % 8} for t in lo])):
        st = St(pqv, oracle, b["data"], b["built"], b["lists"], b["group"], fvalues=b["tenant"], shared=shared)
        try:
            st.check(q, k, None, 1, 64, kind, sp, premise=lambda u: len(set(u.tolist())) >= 4, what="mask")
            st.check(q, k, 2, 2, 64, kind, sp, forms=("device",), what="mask grouped")
        finally:
            st.close()


def test_cosine_and_wide_rows(pqv, oracle):
    """PQV_COSINE through the cosine layout (the depth rule over normalised centroids and queries), on 2048 x 256 (CG = 64)"""
    from cosine_ref import normalise
    rng = np.random.default_rng(267)
    data = rng.random((2048, 256), dtype=np.float32)
    q = rng.random((8, 256), dtype=np.float32)
    built = oracle.build_index(data, n_clusters=8, max_iters=5, workers=1)
    lists = built.lists()
    group = (rng.integers(0, 300, 2048) * 3 - 400).astype(np.int64)
    tenant = rng.integers(0, 6, 2048).astype(np.int32)
    st = St(pqv, oracle, data, built, lists, group, fvalues=tenant, shared=rng.random(2048) < 1 / 2)
    try:
        spec = ([0, 1, 2, 3, 4, 5, 0, 1], [1, 1, 3, 3, 5, 5, 0, 4])
        st.check(q, 60, None, 1, 8, RANGE, spec, premise=lambda u: len(set(u.tolist())) >= 2, what="dim 256")
        st.check(q, 60, 2, 1, 8, RANGE, spec, forms=("device",), what="dim 256 grouped")
        st.order_oidx = oracle.index_from_parts(256, normalise(np.asarray(built.centroids, np.float32).reshape(-1, 256)), lists)
        st.order_q = normalise
        st.check(q, 60, None, 1, 8, RANGE, spec, metric=pqv.PQV_COSINE, premise=lambda u: len(set(u.tolist())) >= 2, what="cosine")
        st.check(q, 60, 2, 1, 8, None, None, metric=pqv.PQV_COSINE, forms=("device",), what="cosine grouped")
    finally:
        st.close()


def test_counters_and_determinism(eq_case):
    """the counters advance as for the per-u twin calls' matching queries; the same device call twice gives identical bytes"""
    c, st = eq_case
    q, k, p0, P = c["queries"], c["k"], c["nprobe"], c["max_nprobe"]
    names = ("queries", "candidate_rows", "embeddings_fetched")
    for m in (None, 3):
        want = dict.fromkeys(names, 0)
        for u in sorted(set(c["used"].tolist())):
            sel = np.flatnonzero(c["used"] == u)
            spec = [c["spec"][i] for i in sel]
            before = st.s.counters()
            st.host(q[sel], k, m, u, c["kind"], spec)
            after = st.s.counters()
            for nme in names:
                want[nme] += after[nme] - before[nme]
        for form in ("host", "device"):
            before = st.s.counters()
            getattr(st, form)(q, k, m, p0, c["kind"], c["spec"], max_nprobe=P)
            after = st.s.counters()
            assert {nme: after[nme] - before[nme] for nme in names} == want, (form, m)
        a = st.device(q, k, m, p0, c["kind"], c["spec"], max_nprobe=P, raw=True)
        b = st.device(q, k, m, p0, c["kind"], c["spec"], max_nprobe=P, raw=True)
        assert a == b


def test_refusals(pqv, oracle, eq_case):
    c, st = eq_case
    q = c["queries"][:2]
    spec = c["spec"][:2]

    def refused(text, fn):
        with pytest.raises(pqv.PqvError, match=text) as e:
            fn()
        assert e.value.code == UNSUPPORTED, e.value

    dot = "PQV_DOT is not supported by keyed and distinct calls"
    d_lim = "pqv_topk_distinct_expand takes k <= 1024 and at most 1024 probed lists per query"
    g_lim = "pqv_topk_grouped_expand takes k \\* group_size <= 1024 and at most 1024 probed lists per query"
    for form in (st.host, st.device):
        refused(dot, lambda: form(q, 5, None, 1, None, None, max_nprobe=4, metric=pqv.PQV_DOT))
        refused(dot, lambda: form(q, 5, 2, 1, c["kind"], spec, max_nprobe=4, metric=pqv.PQV_DOT))
        refused(d_lim, lambda: form(q, 1025, None, 1, c["kind"], spec, max_nprobe=4))
        refused(g_lim, lambda: form(q, 205, 5, 1, None, None, max_nprobe=4))             # k * m = 1025
    # the product in 64 bits (2^31 * 2 wraps to 0 in 32): the raw symbols, whose limits come before any buffer is looked at
    from pq_vector_amd import _ffi
    lib = _ffi.lib()
    small = np.zeros(8, np.float32)
    f32p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    rc = lib.pqv_topk_grouped_expand(st.s._h, st.gkeys._h, None, None, None, small.ctypes.data_as(f32p), 0, q.shape[1], 2 ** 31, 2, 1, 4, 0, 0,
                                     small.view(np.uint32).ctypes.data_as(u32p), small.ctypes.data_as(f32p), None, None, None, None, None)
    assert rc == UNSUPPORTED and b"pqv_topk_grouped_expand takes k * group_size <= 1024" in lib.pqv_last_error()
    rc = lib.pqv_topk_grouped_expand_device(st.s._h, st.gkeys._h, None, None, None, None, 0, 2 ** 31, 2, 1, 4, 0, 0, None, None, None, None,
                                            None, None, None, None)
    assert rc == UNSUPPORTED and b"pqv_topk_grouped_expand takes k * group_size <= 1024" in lib.pqv_last_error()


def test_refusal_beyond_1024_probed_lists_and_tables(pqv, oracle):
    def refused(text, fn):
        with pytest.raises(pqv.PqvError, match=text) as e:
            fn()
        assert e.value.code == UNSUPPORTED, e.value

    d_lim = "pqv_topk_distinct_expand takes k <= 1024 and at most 1024 probed lists per query"
    g_lim = "pqv_topk_grouped_expand takes k \\* group_size <= 1024 and at most 1024 probed lists per query"
    # an index of 1025 one-row lists
    data, oidx, lists = _line_index(oracle, 4, [1] * 1025)
    wide = St(pqv, oracle, data, oidx, lists, np.arange(1025, dtype=np.int64))
    try:
        for form in (wide.host, wide.device):
            refused(d_lim, lambda: form(data[:2], 5, None, 1, None, None, max_nprobe=1025))
            refused(g_lim, lambda: form(data[:2], 5, 2, 1, None, None, max_nprobe=2000))
        wide.check(data[:2], 5, None, 1, 1024, premise=lambda u: (u == 5).all(), forms=("device",), what="1024 lists")
    finally:
        wide.close()
    # a table searcher
    from test_gpu_table import Table
    rng = np.random.default_rng(12)
    t = Table(pqv, oracle, rng, [300, 200], [4, 3], 8)
    col = pqv.Column.upload(np.arange(len(t.data), dtype=np.int64), None, device=0)
    keys = t.s.row_keys(col)
    col.close()
    tq = rng.random((1, 8), dtype=np.float32)
    refused("pqv_topk_distinct_expand does not take table searchers", lambda: t.s.topk_distinct(tq, 2, 1, keys, max_nprobe=2))
    refused("pqv_topk_grouped_expand does not take table searchers", lambda: t.s.topk_grouped(tq, 2, 2, 1, keys, max_nprobe=2))
    keys.close()


def test_builders(pqv, eq_case):
    c, st = eq_case
    q = c["queries"][3]
    st.s.attach_column("doc", pqv.Column.upload(c["group"], None, device=0), own=True)
    allow = cases.doc_mask(np.random.default_rng(8), c["group"], 1 / 8)
    exp = st.s.topk_distinct(q, 10, 1, st.gkeys, max_nprobe=16)
    got = pqv.TopkBuilder(st.s, q).k(10).nprobe(1).distinct_on("doc").max_nprobe(16).search()
    n = int(exp[3][0])
    assert [(r.row_idx, r.key) for r in got] == list(zip(exp[0][0, :n].tolist(), exp[2][0, :n].tolist())) and n == 10
    m = st.s.row_mask(allow)
    exp = st.s.topk_distinct(q, 10, 1, st.gkeys, mask=m, max_nprobe=16)
    plain = st.s.topk_distinct(q, 10, 1, st.gkeys, mask=m)
    assert exp[5][0] > 1 and exp[3][0] > plain[3][0]              # the expansion found more documents than the fixed depth
    got = pqv.TopkBuilder(st.s, q).k(10).nprobe(1).where(allow).distinct_on("doc").max_nprobe(16).search()
    n = int(exp[3][0])
    assert [(r.row_idx, r.key) for r in got] == list(zip(exp[0][0, :n].tolist(), exp[2][0, :n].tolist()))
    expg = st.s.topk_grouped(q, 10, 3, 1, st.gkeys, mask=m, max_nprobe=16)
    gotg = pqv.TopkBuilder(st.s, q).k(10).nprobe(1).where(allow).distinct_on("doc").group_size(3).max_nprobe(16).search()
    assert len(gotg) == int(expg[4][0]) == n
    for g, res in enumerate(gotg):
        cnt = int(expg[3][0, g])
        assert res.key == expg[2][0, g] and [h.row_idx for h in res.hits] == expg[0][0, g, :cnt].tolist()
    expg = st.s.topk_grouped(q, 10, 3, 1, st.gkeys, max_nprobe=16)
    gotg = pqv.TopkBuilder(st.s, q).k(10).nprobe(1).distinct_on("doc").group_size(3).max_nprobe(16).search()
    assert [r.key for r in gotg] == expg[2][0, :int(expg[4][0])].tolist()
    m.close()
