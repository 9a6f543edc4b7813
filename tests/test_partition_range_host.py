"""Range search over a key partition (pqv.h: pqv_range_search_partition), host side: the numpy restatement
(tests/partition_range_ref.py) on a hand-written example, against mask_ref's masked range run over the one-list index S1 and against
the partition top-k restatement (the contract's two equivalences), the conditions on the GPU tests' inputs
(tests/partition_range_cases.py), the ABI surface, the validation order -- all of it before any device use -- and the Python
wrapper's argument handling."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import key_filter_ref as kf
import mask_ref
import partition_cases as pc
import partition_range_cases as prc
import partition_range_ref as prr
import partition_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "pqv_range_search_partition"
INF = np.float32(np.inf)


@pytest.fixture(scope="module")
def lib():
    from pq_vector_amd import _ffi
    return _ffi.lib()


def test_restatement_is_the_contract():
    # (the example of test_partition_host.py::test_restatement_is_the_contract)
    col = np.array([3, -1, 3, 7, -1, 3, 0, 7, 3], np.int32)
    valid = np.array([1, 1, 0, 1, 1, 1, 1, 0, 1], np.uint8)
    rows, keys = pr.build(col, valid, [8, 0, 1, 2, 3, 4, 5, 6])
    assert rows.tolist() == [1, 4, 6, 0, 5, 8, 3] and keys.tolist() == [-1, -1, 0, 3, 3, 3, 7]
    d = np.array([5, 1, 9, 2, 1, 5, 0, 0, 4], np.float32)
    allow = np.ones(9, bool)
    allow[6] = False
    # RANGE [-1, 3]: candidates 1 4 6 0 5 8 at positions 0..5, row 6 masked out; positions stay the unmasked ones

    def call(radius, **kw):
        r, dd, nw, nc, cons = prr.range_query(rows, keys, kf.RANGE, [-1], [3], 0, d, radius, allow=allow, **kw)
        assert (nc, cons) == (6, 5) and r.dtype == np.uint32 and dd.dtype == np.float32
        return r.tolist(), dd.tolist(), nw

    assert call(4) == ([1, 4, 8], [1, 1, 4], 3), "inclusive, ordered by (distance, position)"
    assert call(np.nextafter(np.float32(4), np.float32(0))) == ([1, 4], [1, 1], 2)
    assert call(2, sqrt_out=True) == ([1, 4, 8], [1, 1, 2], 3), "the hit test is on the output scale"
    assert call(-1) == ([], [], 0) and call(-INF) == ([], [], 0)
    assert call(INF) == ([1, 4, 8, 0, 5], [1, 1, 4, 5, 5], 5)
    assert call(INF, max_results=2) == ([1, 4], [1, 1], 5), "n_within counts before max_results"
    assert call(INF, max_results=9) == call(INF)
    # unmasked: row 6 (distance 0) comes first; n_candidates is the same
    r, dd, nw, nc, cons = prr.range_query(rows, keys, kf.RANGE, [-1], [3], 0, d, 1)
    assert (r.tolist(), dd.tolist(), nw, nc, cons) == ([6, 1, 4], [0, 1, 1], 3, 6, 6)
    # an absent key, an inverted range, an empty set: nothing, and no candidates
    for kind, a, b in ((kf.EQ, [2 ** 32 + 3], None), (kf.RANGE, [3], [0]), (kf.IN, [0, 0], [])):
        assert prr.range_query(rows, keys, kind, a, b, 0, d, INF)[2:] == (0, 0, 0)
    # PQV_COSINE: out = 0.5 d2 whatever sqrt_out
    for so in (False, True):
        r, dd, nw, _, _ = prr.range_query(rows, keys, kf.RANGE, [-1], [3], 0, d, 0.5, "cos", so, allow)
        assert (r.tolist(), dd.tolist(), nw) == ([1, 4], [0.5, 0.5], 2)
    # PQV_DOT: signed distances, sqrt_out ignored, a negative radius keeps what lies below it
    for so in (False, True):
        r, dd, nw, _, _ = prr.range_query(rows, keys, kf.RANGE, [-1], [3], 0, -d, -4.5, "dot", so, allow)
        assert (r.tolist(), dd.tolist(), nw) == ([0, 5], [-5, -5], 2)
    assert prr.range_query(rows, keys, kf.RANGE, [-1], [3], 0, -d, 0, "dot", allow=allow)[2] == 5
    # a NaN distance is never a hit, not even at +inf
    dn = d.copy()
    dn[4] = np.nan
    r, dd, nw, nc, cons = prr.range_query(rows, keys, kf.RANGE, [-1], [3], 0, dn, INF, allow=allow)
    assert (r.tolist(), nw, nc, cons) == ([1, 8, 0, 5], 4, 6, 5)
    # the CSR form
    lims, r, dd, nw, nc, cons = prr.range_batch(rows, keys, kf.EQ, [3, 9, -1], None, np.stack([d, d, d]), 4.5)
    assert lims.tolist() == [0, 1, 1, 3] and r.tolist() == [8, 1, 4] and nw.tolist() == [1, 0, 2] and nc.tolist() == [3, 0, 2] and cons == 5
    assert lims.dtype == nw.dtype == nc.dtype == np.uint64


@pytest.mark.parametrize("name", ["4096x128", "2048x32-seq"])
def test_restatement_equals_the_masked_range_restatement_on_the_one_list_index(name):
    """Equivalence (b).  S1: one list = all indexed rows ascending.  There key_filter_ref's M_q through mask_ref.masked_range is
    pqv_range_search_masked's restatement (nprobe = 1, no cap), and -- no two rows tie -- the partition's answer, EQ, RANGE and IN."""
    c = pc.Case(name)
    indexed = np.setdiff1d(np.arange(c.n), np.arange(5, c.n, 37))        # (as after a remove)
    shared = np.random.default_rng(9).random(c.n) < 0.5
    compared = 0
    for col, (values, valid) in c.columns.items():
        part = c.partition(col, indexed)
        for flt in c.filters(col):
            _, kind, a, b = flt
            for allow, sqrt_out in ((None, False), (shared, True)):
                m = [kf.allowed_for(values, valid, kind, a, b, q, allow) for q in range(c.nq)]
                for label, radius in prc.radii(prc.reference(c, part, flt, INF, sqrt_out, allow)):
                    for max_results in (0, 5):
                        lims, rows, dist, nw, nc, _ = prc.reference(c, part, flt, radius, sqrt_out, allow, max_results)
                        for q in range(c.nq):
                            er, ed, enw, _ = mask_ref.masked_range(indexed.astype(np.uint32), m[q], c.data, c.queries[q], radius, c.metric,
                                                                   sqrt_out, max_results=max_results)
                            lo, hi = int(lims[q]), int(lims[q + 1])
                            assert nw[q] == enw and (rows[lo:hi] == er).all(), (col, flt[0], label, q)
                            assert (dist[lo:hi].view(np.uint32) == ed.view(np.uint32)).all()
                            assert nc[q] == int(kf.allowed_for(values, valid, kind, a, b, q)[indexed].sum())
                            compared += len(er)
    assert compared > 10000


def _cases(oracle):
    yield from ((pc.Case(n), prc.COLUMNS) for n in pc.SHAPES)
    yield from ((prc.LongCase(n, oracle), ("i32", "i64")) for n in prc.LONG_SHAPES)
    yield prc.TieCase(), ("key",)


def test_restatement_at_infinity_is_the_topk_restatement(oracle):
    """Equivalence (a): radius = +inf and max_results = k is pr.topk's first n_found rows -- ties included"""
    for c, cols in _cases(oracle):
        shared = np.random.default_rng(3).random(c.n) < 0.5
        for col in cols:
            part = c.partition(col)
            for flt in c.filters(col):
                for k, sqrt_out, allow in ((1, False, None), (10, True, shared), (300, False, shared), (1024, True, None)):
                    lims, rows, dist, nw, nc, cons = prc.reference(c, part, flt, INF, sqrt_out, allow, k)
                    tr, td, tnf, tnc, tcons = pr.topk_batch(part[0], part[1], flt[1], flt[2], flt[3], c.d, k, c.kind, sqrt_out, allow)
                    assert (nc == tnc).all() and cons == tcons and (np.diff(lims.astype(np.int64)) == tnf).all()
                    for q in range(c.nq):
                        lo, hi = int(lims[q]), int(lims[q + 1])
                        assert (rows[lo:hi] == tr[q, :tnf[q]]).all() and (dist[lo:hi].view(np.uint32) == td[q, :tnf[q]].view(np.uint32)).all()
                        assert nw[q] >= tnf[q]


def test_radii_are_not_vacuous(oracle):
    """per (case, filter): no hit below, every considered row at +inf, the median keeps some and drops some, and the boundary
    radius -- exactly the j-th nearest considered distance of query 0 -- keeps exactly j + 1 rows of query 0"""
    boundaries = splits = 0
    kinds = set()
    for c, cols in _cases(oracle):
        if isinstance(c, prc.TieCase):
            continue
        for col in cols:
            part = c.partition(col)
            for flt in c.filters(col):
                kinds.add(flt[1])
                for sqrt_out, allow in ((False, None), (True, np.random.default_rng(3).random(c.n) < 0.5)):
                    ref_inf = prc.reference(c, part, flt, INF, sqrt_out, allow)
                    assert int(ref_inf[3].sum()) == ref_inf[5], "+inf keeps every considered row (no NaN distance)"
                    for label, radius in prc.radii(ref_inf):
                        assert not np.isnan(radius)
                        nw = prc.reference(c, part, flt, radius, sqrt_out, allow)[3]
                        if label == "below":
                            assert nw.sum() == 0
                        elif label == "median" and ref_inf[5] > 1:
                            assert 0 < nw.sum() <= ref_inf[5]
                            splits += int(nw.sum() < ref_inf[5])
                        elif prc.boundary_j(label) is not None:
                            assert nw[0] == prc.boundary_j(label) + 1, (c.name, col, flt[0], label)
                            boundaries += 1
                        if c.kind == "dot" and np.isfinite(radius):
                            assert radius < 0, "PQV_DOT: negative radii that still keep rows"
    assert kinds == {kf.EQ, kf.RANGE, kf.IN} and boundaries > 100 and splits > 100
    # a 1024-value IN set is among the filters
    c = pc.Case("2048x256")
    assert {max(np.diff(c.filters(col)[2][2])) for col in ("t64", "distinct", "skew")} == {1024}


def test_big_case_reaches_the_merge_passes():
    c = prc.BigCase()
    part = c.partition()
    assert len(part[0]) == c.n == 10000 and (c.keys == prc.BIG["big_key"]).sum() == prc.BIG["big_rows"]
    assert max(len(np.unique(row)) for row in c.d) < 200, "integer rows: equal distances all the way down"
    two = one = 0
    for flt in c.filters():
        nw = prc.reference(c, part, flt, INF)[3]
        two += int((nw > 2 * prc.RANGE_SMALL).sum())
        nwm = prc.reference(c, part, flt, INF, allow=c.shared)[3]
        one += int(((nwm > prc.RANGE_SMALL) & (nwm <= 2 * prc.RANGE_SMALL)).sum())
        assert (nw[nw > 0] != nwm[nw > 0]).all()
    assert two >= 4 and one >= 4, "segments of two merge passes, and of one under the mask"
    # max_results cuts inside a long segment, at the tile's edge and one beyond
    flt = c.filters()[0]
    full = prc.reference(c, part, flt, INF)
    assert full[3][0] == prc.BIG["big_rows"]
    for mr in prc.BIG_MAX_RESULTS:
        lims, rows, dist, nw, _, _ = prc.reference(c, part, flt, INF, max_results=mr)
        assert lims[1] == min(mr, prc.BIG["big_rows"]) and (nw == full[3]).all()
        assert (rows[:int(lims[1])] == full[1][:int(lims[1])]).all()
    # a finite radius in the middle of the ties
    med = prc.radii(full)[2][1]
    nw = prc.reference(c, part, flt, med)[3]
    assert prc.RANGE_SMALL < nw[0] < prc.BIG["big_rows"]


def test_symbol_exported_bound_and_in_every_binding(lib):
    from pq_vector_amd import _ffi
    import pq_vector_amd as pqv
    hdr = open(os.path.join(ROOT, "include", "pqv.h")).read()
    sys_rs = open(os.path.join(ROOT, "bindings", "rust", "src", "sys.rs")).read()
    raw = C.CDLL(_ffi.LIB_PATH)
    assert hasattr(raw, SYMBOL) and SYMBOL in _ffi.SIGNATURES
    assert getattr(lib, SYMBOL).argtypes == _ffi.SIGNATURES[SYMBOL][1]
    assert re.search(r"\b%s\s*\(" % SYMBOL, hdr) and re.search(r"pub fn %s\(" % SYMBOL, sys_rs)
    # pqv_range_search_filtered's arity less keys (a partition instead), nprobe and max_candidates
    assert len(_ffi.SIGNATURES[SYMBOL][1]) == len(_ffi.SIGNATURES["pqv_range_search_filtered"][1]) - 2
    for f, needle in (("bindings/rust/src/lib.rs", "pub fn range_search_partition"), ("bindings/rust/src/lib.rs", "sys::" + SYMBOL),
                      ("pq-vector_amd/host/pqv.hpp", SYMBOL + "("), ("pq-vector_amd/csrc/Makefile", "kernels_partition_range.o"),
                      ("pq-vector_amd/csrc/Makefile", "kernels_partition_range.hip"),
                      ("pq-vector_amd/csrc/kernels_all.hip", "kernels_partition_range.hip"),
                      ("pq-vector_amd/csrc/kernels.h", "touch_partition_range"), ("pq-vector_amd/__init__.py", "range_search_partition"),
                      ("README.md", "range_search_partition"), ("DESIGN.md", SYMBOL), ("include/pqv.h", '"partition_range_bytes"')):
        assert needle in open(os.path.join(ROOT, f)).read(), (f, needle)
    assert callable(pqv.Searcher.range_search_partition)
    assert "range search over a partition" not in hdr, "no longer out of scope"
    assert lib.pqv_abi_version() == 101


def test_c_abi_validates_in_the_stated_order_before_device_use(lib):
    from pq_vector_amd import _ffi
    inv = _ffi.PQV_ERR_INVALID
    fake = C.c_void_p(8)                 # never dereferenced: every check below comes before a handle is read
    zeros = (C.c_uint8 * 4096)()         # a handle whose owner is nobody: read by the ownership check only
    other = C.cast(zeros, C.c_void_p)
    nq = 2
    q = (C.c_float * (4 * nq))()
    lims, rows, dist = _ffi.u64p(), _ffi.u32p(), _ffi.f32p()

    def call(s, part, f, radius=1.0, mask=None):
        return lib.pqv_range_search_partition(s, part, f, mask, q, nq, 4, radius, 0, 0, 1, C.byref(lims), C.byref(rows), C.byref(dist), None, None)

    def flt(kind, a, b):
        return C.byref(_ffi.KeyFilter(kind, 0, C.cast(a, C.c_void_p) if a is not None else None,
                                      C.cast(b, C.c_void_p) if b is not None else None))

    def err(rc, text, code=inv):
        assert rc == code and text in lib.pqv_last_error(), (rc, lib.pqv_last_error())

    i64 = lambda *v: (C.c_int64 * len(v))(*v)       # noqa: E731
    u64 = lambda *v: (C.c_uint64 * len(v))(*v)      # noqa: E731
    big = i64(*range(1025))
    good = flt(_ffi.PQV_KEY_EQ, i64(1, 2), None)
    nan = float("nan")
    err(call(None, None, None), b"searcher must not be NULL")
    err(call(None, fake, good, nan), b"searcher must not be NULL")
    err(call(fake, None, None), b"key partition must not be NULL")
    err(call(fake, None, good, nan), b"key partition must not be NULL")
    err(call(fake, fake, None, nan), b"filter must not be NULL")
    err(call(fake, fake, flt(3, i64(1, 2), None)), b"unknown key filter kind 3")
    err(call(fake, fake, flt(_ffi.PQV_KEY_EQ, None, None)), b"query keys must not be NULL")
    err(call(fake, fake, flt(_ffi.PQV_KEY_RANGE, i64(1, 2), None)), b"query keys must not be NULL")
    err(call(fake, fake, flt(_ffi.PQV_KEY_IN, None, i64(1, 2))), b"query keys must not be NULL")
    # the host descriptor checks of pqv_topk_filtered
    err(call(fake, fake, flt(_ffi.PQV_KEY_IN, u64(1, 1, 2), i64(1, 2))), b"query key sets must start at 0 and not decrease")
    err(call(fake, fake, flt(_ffi.PQV_KEY_IN, u64(0, 2, 1), i64(1, 2))), b"query key sets must start at 0 and not decrease")
    err(call(fake, fake, flt(_ffi.PQV_KEY_IN, u64(0, 0, 1025), big)), b"a query key set takes at most 1024 values")
    err(call(fake, fake, flt(_ffi.PQV_KEY_IN, u64(0, 2, 4), i64(1, 2, 4, 4)), nan), b"query key sets must be strictly ascending")
    # ... ahead of the ownership checks, which come ahead of the radius
    for ok in (good, flt(_ffi.PQV_KEY_RANGE, i64(1, 2), i64(0, 9)), flt(_ffi.PQV_KEY_IN, u64(0, 1024, 1024), big)):
        err(call(fake, other, ok), b"key partition belongs to another searcher")
        err(call(fake, other, ok, nan, mask=other), b"key partition belongs to another searcher")
    assert not lims and not rows and not dist, "no buffer is handed out by a refused call"


def test_python_wrapper_checks_its_arguments_before_device_use():
    import pq_vector_amd as pqv
    s = object.__new__(pqv.Searcher)       # no device here: the checks must come before the library is asked
    s._columns = {}
    q = np.zeros((2, 4), np.float32)
    fake = pqv.KeyPartition(8, s)          # (a handle that is never handed to the library)
    try:
        with pytest.raises(pqv.PqvError, match="part must be a KeyPartition"):
            s.range_search_partition(q, 1.0, pqv.RowKeys(None, s), query_keys=[1, 2])
        with pytest.raises(pqv.PqvError, match="key partition must not be NULL"):
            s.range_search_partition(q, 1.0, pqv.KeyPartition(None, s), query_keys=[1, 2])
        with pytest.raises(pqv.PqvError, match="query keys must not be NULL"):
            s.range_search_partition(q, 1.0, fake)
        with pytest.raises(pqv.PqvError, match="mutually exclusive"):
            s.range_search_partition(q, 1.0, fake, query_keys=[1, 2], query_key_ranges=([1, 2], [3, 4]))
        with pytest.raises(pqv.PqvError, match="1 query keys for 2 queries"):
            s.range_search_partition(q, 1.0, fake, query_keys=[1])
        with pytest.raises(pqv.PqvError, match="must be a pair"):
            s.range_search_partition(q, 1.0, fake, query_key_ranges=5)
        with pytest.raises(pqv.PqvError, match="3 query key sets for 2 queries"):
            s.range_search_partition(q, 1.0, fake, query_key_sets=[[1], [2], [3]])
        with pytest.raises(ValueError, match="at most 1024 values"):
            s.range_search_partition(q, 1.0, fake, query_key_sets=[[1], range(2000)])
        with pytest.raises(pqv.PqvError, match="mask must be a RowMask"):
            s.range_search_partition(q, 1.0, fake, query_keys=[1, 2], mask=np.ones(4, bool))
        with pytest.raises(pqv.PqvError, match="row mask must not be NULL"):
            s.range_search_partition(q, 1.0, fake, query_keys=[1, 2], mask=pqv.RowMask(None, s))
        with pytest.raises(pqv.PqvError, match="radius must not be NaN"):
            s.range_search_partition(q, float("nan"), fake, query_keys=[1, 2])
        with pytest.raises(pqv.PqvError, match="max_results must be >= 0"):
            s.range_search_partition(q, 1.0, fake, query_keys=[1, 2], max_results=-1)
    finally:
        fake._h = None
        s._h = None
