"""Distinct / grouped top-k under a per-query key filter, host side: the ABI surface, the full order of the argument checks with
handles that are never dereferenced, the numpy restatement (tests/distinct_filter_ref.py) on a hand-made example, and the
non-vacuity of the inputs the GPU cases use (tests/distinct_filter_cases.py), checked with that restatement over the C oracle's
candidates.  The checks that need a real searcher are in tests/test_gpu_distinct_filter.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import distinct_filter_cases as cases
import distinct_filter_ref as ref
import distinct_ref
from test_gpu_mask import SHAPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pqv_topk_distinct_filtered", "pqv_topk_distinct_filtered_device", "pqv_topk_grouped_filtered",
               "pqv_topk_grouped_filtered_device")


@pytest.fixture(scope="module")
def lib():
    from pq_vector_amd import _ffi
    return _ffi.lib()


def test_symbols_exported_bound_and_in_every_binding(lib):
    from pq_vector_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "pqv.h")).read()
    sys_rs = open(os.path.join(ROOT, "bindings", "rust", "src", "sys.rs")).read()
    raw = C.CDLL(_ffi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _ffi.SIGNATURES
        assert getattr(lib, name).argtypes == _ffi.SIGNATURES[name][1]
        assert re.search(r"\b%s\s*\(" % name, hdr)
        assert re.search(r"pub fn %s\(" % name, sys_rs)
        # the twin plus filter_keys and filter
        twin = name.replace("_filtered", "")
        assert len(_ffi.SIGNATURES[name][1]) == len(_ffi.SIGNATURES[twin][1]) + 2
        assert _ffi.SIGNATURES[name][1][3] == C.POINTER(_ffi.KeyFilter)
    for f, needle in (("bindings/rust/src/lib.rs", "pub fn topk_distinct_filtered("), ("bindings/rust/src/lib.rs", "pub fn topk_grouped_filtered("),
                      ("pq-vector_amd/host/pqv.hpp", "void topk_distinct_filtered("), ("pq-vector_amd/host/pqv.hpp", "void topk_grouped_filtered(")):
        assert needle in open(os.path.join(ROOT, f)).read(), (f, needle)
    assert "a per-query key filter combined with" not in hdr          # no longer out of the twins' scope
    assert lib.pqv_abi_version() == 101


def test_c_abi_validates_in_the_contract_s_order_before_device_use(lib):
    from pq_vector_amd import _ffi
    inv = _ffi.PQV_ERR_INVALID
    fake = C.c_void_p(8)         # never dereferenced: every NULL and zero check comes first
    q = (C.c_float * 4)()
    rows, dist, grp, cnt = (C.c_uint32 * 4)(), (C.c_float * 4)(), (C.c_int64 * 2)(), (C.c_uint32 * 2)()
    keys = (C.c_int64 * 1)(3)
    lims_bad, lims_dec = (C.c_uint64 * 2)(1, 1), (C.c_uint64 * 3)(0, 2, 1)
    lims_ok, vals_unsorted = (C.c_uint64 * 2)(0, 2), (C.c_int64 * 2)(5, 5)
    lims_long = (C.c_uint64 * 2)(0, 1025)

    def flt(kind, a, b=None):
        return C.byref(_ffi.KeyFilter(kind, 0, C.cast(a, C.c_void_p).value if a is not None else None,
                                      C.cast(b, C.c_void_p).value if b is not None else None))

    ok = flt(_ffi.PQV_KEY_EQ, keys)

    def d_host(s, g, fk, f, k=2, m=None, nq=1):
        return lib.pqv_topk_distinct_filtered(s, g, fk, f, None, q, nq, 4, k, 1, 0, 0, 1, rows, dist, grp, None, None)

    def d_device(s, g, fk, f, k=2, m=None, nq=1):
        return lib.pqv_topk_distinct_filtered_device(s, g, fk, f, None, None, nq, k, 1, 0, 0, 1, None, None, None, None, None, None)

    def g_host(s, g, fk, f, k=2, m=2, nq=1):
        return lib.pqv_topk_grouped_filtered(s, g, fk, f, None, q, nq, 4, k, m, 1, 0, 0, 1, rows, dist, grp, cnt, None, None)

    def g_device(s, g, fk, f, k=2, m=2, nq=1):
        return lib.pqv_topk_grouped_filtered_device(s, g, fk, f, None, None, nq, k, m, 1, 0, 0, 1, None, None, None, None, None, None, None)

    def refused(rc, text):
        assert rc == inv and text in lib.pqv_last_error(), lib.pqv_last_error()

    for call in (d_host, d_device, g_host, g_device):
        grouped = call in (g_host, g_device)
        host = call in (d_host, g_host)
        # 1 - 4: the NULLs, each ahead of everything behind it
        refused(call(None, None, None, None, k=0, m=0), b"searcher must not be NULL")
        refused(call(fake, None, None, None, k=0, m=0), b"row keys must not be NULL")
        refused(call(fake, fake, None, None, k=0, m=0), b"a key filter needs row keys")
        refused(call(fake, fake, None, ok, k=0, m=0), b"a key filter needs row keys")
        refused(call(fake, fake, fake, None, k=0, m=0), b"filter must not be NULL")
        # 5: the descriptor checks of pqv_topk_filtered, ahead of k
        refused(call(fake, fake, fake, flt(7, keys), k=0, m=0), b"unknown key filter kind 7")
        refused(call(fake, fake, fake, flt(_ffi.PQV_KEY_EQ, None), k=0, m=0), b"query keys must not be NULL")
        refused(call(fake, fake, fake, flt(_ffi.PQV_KEY_RANGE, keys, None), k=0, m=0), b"query keys must not be NULL")
        if host:         # (a set filter is validated in full by the host forms only)
            refused(call(fake, fake, fake, flt(_ffi.PQV_KEY_IN, lims_bad, keys), k=0, m=0), b"query key sets must start at 0 and not decrease")
            refused(call(fake, fake, fake, flt(_ffi.PQV_KEY_IN, lims_dec, vals_unsorted), k=0, m=0, nq=2),
                    b"query key sets must start at 0 and not decrease")
            refused(call(fake, fake, fake, flt(_ffi.PQV_KEY_IN, lims_long, keys), k=0, m=0), b"a query key set takes at most 1024 values")
            refused(call(fake, fake, fake, flt(_ffi.PQV_KEY_IN, lims_ok, vals_unsorted), k=0, m=0), b"query key sets must be strictly ascending")
        # 6, 7: the zeros, still before a handle is read
        refused(call(fake, fake, fake, ok, k=0, m=0), b"k must be > 0")
        if grouped:
            refused(call(fake, fake, fake, ok, k=2, m=0), b"group_size must be > 0")
        # nq == 0: the descriptor's arrays are not asked for, the zeros still are
        refused(call(fake, fake, fake, flt(_ffi.PQV_KEY_EQ, None), k=0, nq=0), b"k must be > 0")


def test_python_layer_without_a_device():
    import pq_vector_amd as pqv
    s = object.__new__(pqv.Searcher)       # no device here: the checks must come before the library is asked
    s._h, s.dim, s.n_clusters, s._columns = None, 4, 2, {}
    qq = np.zeros((2, 4), np.float32)
    keys, closed = pqv.RowKeys(C.c_void_p(8), s), pqv.RowKeys(None, s)
    try:
        for call in (lambda **kw: s.topk_distinct(qq, 2, 1, keys, **kw), lambda **kw: s.topk_grouped(qq, 2, 2, 1, keys, **kw),
                     lambda **kw: s.topk_distinct_device(8, 2, 2, 1, keys, 8, 8, **kw),
                     lambda **kw: s.topk_grouped_device(8, 2, 2, 2, 1, keys, 8, 8, **kw)):
            with pytest.raises(pqv.PqvError, match="query_keys needs filter_keys="):
                call(query_keys=[1, 2])
            with pytest.raises(pqv.PqvError, match="query_key_sets needs filter_keys="):
                call(query_key_sets=[[1], [2]])
            with pytest.raises(pqv.PqvError, match="filter_keys= needs query_keys=, query_key_ranges= or query_key_sets="):
                call(filter_keys=keys)
            with pytest.raises(pqv.PqvError, match="query_keys and query_key_ranges are mutually exclusive"):
                call(filter_keys=keys, query_keys=[1, 2], query_key_ranges=([1, 2], [3, 4]))
            with pytest.raises(pqv.PqvError, match="row keys must not be NULL"):
                call(filter_keys=closed, query_keys=[1, 2])
    finally:
        keys._h = None          # (a made-up handle: nothing to free)


def test_restatement_on_a_hand_made_example():
    # test_distinct_host's example: 12 rows of dimension 1, the query at 0: d2 = value^2; the candidate sequence is a permutation
    data = np.array([3, 1, 1, 2, 5, 1, 4, 2, 0.5, 6, 2, 7], np.float32).reshape(12, 1)
    doc = np.array([10, 20, 30, 20, 10, 30, 40, 50, 60, 60, 40, 70], np.int64)
    tenant = np.array([1, 2, 1, 1, 1, 2, 2, 1, 2, 1, 1, 3], np.int32)
    cand = np.array([4, 5, 2, 1, 0, 3, 7, 6, 8, 9, 10, 11], np.uint32)
    q = np.zeros(1, np.float32)
    # unfiltered: S = 8 | 5 2 1 | 3 7 10 | 0 | 6 | 4 | 9 | 11 -> docs 60 (row 8), 30 (row 5), 20 (row 1), 50 (row 7), 40 (row 10), 10 (row 0), 70
    # tenant 1: rows 0 2 3 4 7 9 10 pass.  Doc 60's nearest row 8 fails: row 9 (d2 36) represents it; doc 30: row 2, not row 5;
    # doc 20: row 3 (d2 4), not row 1
    r, d2, g, nc, ncons = ref.distinct_topk(cand, doc, None, tenant, None, ref.EQ, [1], 0, None, data, q[0:1], 10)
    assert r.tolist() == [2, 3, 7, 10, 0, 9] and g.tolist() == [30, 20, 50, 40, 10, 60] and d2.tolist() == [1, 4, 4, 4, 9, 36]
    assert nc == 12 and ncons == 7
    # filtering AFTER the deduplication would return rows 7, 10, 0 only
    ur, _, _, _, _ = distinct_ref.distinct_topk(cand, doc, None, None, data, q, 10)
    assert [x for x in ur.tolist() if tenant[x] == 1] == [7, 10, 0]
    assert ref.vacuity(cand, doc, None, tenant, None, ref.EQ, [1], 0, None, data, q, 10) == (True, True, False)
    assert ref.vacuity(cand, doc, None, tenant, None, ref.EQ, [1], 0, None, data, q, 3) == (True, False, True)
    # RANGE [2, 3] and IN {2, 3} are the same rows; NULL filter keys never pass; a shared mask is ANDed in
    a = ref.distinct_topk(cand, doc, None, tenant, None, ref.RANGE, ([2], [3]), 0, None, data, q, 10)
    b = ref.distinct_topk(cand, doc, None, tenant, None, ref.IN, [[3, 2]], 0, None, data, q, 10)
    assert a[0].tolist() == b[0].tolist() == [8, 5, 1, 6, 11] and a[2].tolist() == [60, 30, 20, 40, 70]
    fvalid = np.ones(12, np.uint8); fvalid[8] = 0
    shared = np.ones(12, bool); shared[11] = False
    c = ref.distinct_topk(cand, doc, None, tenant, fvalid, ref.IN, [[2, 3]], 0, shared, data, q, 10)
    assert c[0].tolist() == [5, 1, 6] and c[4] == 3
    # grouped: tenant 1, two rows per doc
    r, d2, g, cnt, nf, nc, _ = ref.grouped_topk(cand, doc, None, tenant, None, ref.EQ, [1], 0, None, data, q, 3, 2)
    assert nf == 3 and g.tolist() == [30, 20, 50] and cnt.tolist() == [1, 1, 1] and r[:, 0].tolist() == [2, 3, 7]
    r, _, g, cnt, nf, _, _ = ref.grouped_topk(cand, doc, None, tenant, None, ref.RANGE, ([1], [2]), 0, None, data, q, 2, 2)
    assert g.tolist() == [60, 30] and r.tolist() == [[8, 9], [5, 2]] and cnt.tolist() == [2, 2]
    # an empty range, an empty set
    assert len(ref.distinct_topk(cand, doc, None, tenant, None, ref.RANGE, ([3], [1]), 0, None, data, q, 4)[0]) == 0
    assert len(ref.distinct_topk(cand, doc, None, tenant, None, ref.IN, [[]], 0, None, data, q, 4)[0]) == 0


@pytest.fixture(scope="module", params=list(SHAPES))
def shape(request, oracle):
    """what test_gpu_mask.Setup builds for the shape, without the searcher"""
    c = SHAPES[request.param]
    rng = np.random.default_rng(11 + c["dim"])
    data = rng.random((c["n"], c["dim"]), dtype=np.float32)
    queries = rng.random((5, c["dim"]), dtype=np.float32)
    built = oracle.build_index(data, n_clusters=c["kc"], max_iters=5, workers=1)
    lists = [np.asarray(l, np.uint32) for l in built.lists()]
    oidx = oracle.index_from_parts(c["dim"], built.centroids, lists)
    return request.param, c, data, queries, oidx


@pytest.mark.parametrize("kind", list(cases.KINDS))
def test_gpu_inputs_are_not_vacuous(shape, kind):
    """For every filter kind at least one query and one (k, nprobe) of the GPU cases meets each of: (a) a group is represented by
    another row than in the unfiltered call, (b) 0 < n_found < k, (c) n_found == k with groups cut off."""
    name, c, data, queries, oidx = shape
    tenant, doc = cases.columns(name, c["n"])
    assert len(np.unique(tenant)) == cases.N_TENANTS and 12 < c["n"] / len(np.unique(doc)) < 20
    # docs span tenants
    assert np.mean([len(np.unique(tenant[doc == d])) for d in np.unique(doc)[:50]]) > 3
    met = [False, False, False]
    for nprobe in (1, 3):
        for qi, q in enumerate(queries):
            cand = oidx.candidate_rows(q, nprobe)
            for k in cases.KS:
                a, b, cc = ref.vacuity(cand, doc, None, tenant, None, cases.KINDS[kind], cases.SPECS[kind], qi, None, data, q, k, metric=c["metric"])
                found = len(ref.distinct_topk(cand, doc, None, tenant, None, cases.KINDS[kind], cases.SPECS[kind], qi, None, data, q, k,
                                              metric=c["metric"])[0])
                met = [met[0] or a, met[1] or (b and found > 0), met[2] or cc]
    assert met == [True, True, True], (name, kind, met)
