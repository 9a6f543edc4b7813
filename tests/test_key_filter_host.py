"""Per-query key filters beyond equality (pqv.h: pqv_key_filter), host side: the numpy restatement of M_q
(tests/key_filter_ref.py) against tests/keyed_ref.py and through tests/mask_ref.py, the ABI surface, the descriptor's validation
-- all of it happens before any device use -- and the Python wrapper's argument handling."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import key_filter_ref as kf
import keyed_ref
import mask_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("pqv_topk_filtered", "pqv_topk_filtered_device", "pqv_range_search_filtered")
NEW_CONSTANTS = {"PQV_KEY_EQ": 0, "PQV_KEY_RANGE": 1, "PQV_KEY_IN": 2, "PQV_KEY_SET_MAX": 1024}


@pytest.fixture(scope="module")
def lib():
    from pq_vector_amd import _ffi
    return _ffi.lib()


def test_restatement_reduces_to_the_keyed_one():
    rng = np.random.default_rng(3)
    for dtype in (np.int32, np.int64):
        col = rng.integers(-4, 5, 200).astype(dtype)
        valid = (rng.random(200) < 0.8).astype(np.uint8)
        shared = rng.random(200) < 0.7
        keys = [-5, -4, 0, 3, 4, 5, 2 ** 40, kf.INT64_MIN, kf.INT64_MAX]
        lims, vals = kf.sets_to_csr([[k] for k in keys])
        for q, key in enumerate(keys):
            for v, m in ((None, None), (valid, None), (valid, shared)):
                want = keyed_ref.allowed_for(col, v, key, m)
                assert (kf.allowed_for(col, v, kf.EQ, keys, None, q, m) == want).all()
                assert (kf.allowed_for(col, v, kf.RANGE, keys, keys, q, m) == want).all()          # lo == hi
                assert (kf.allowed_for(col, v, kf.IN, lims, vals, q, m) == want).all()             # a singleton


def test_restatement_is_the_contract():
    col = np.array([3, -1, 3, 7, -1, 3, 0, 7], np.int32)
    valid = np.array([1, 1, 0, 1, 1, 1, 1, 0], np.uint8)
    mask = np.array([1, 1, 1, 1, 0, 0, 1, 1], bool)
    lo, hi = [0, 4, -1, kf.INT64_MIN, 2 ** 40, 3], [3, 3, -1, kf.INT64_MAX, 2 ** 41, kf.INT64_MAX]
    assert kf.allowed_for(col, None, kf.RANGE, lo, hi, 0).tolist() == [1, 0, 1, 0, 0, 1, 1, 0]           # both ends inclusive
    assert kf.allowed_for(col, valid, kf.RANGE, lo, hi, 0).tolist() == [1, 0, 0, 0, 0, 1, 1, 0]          # a NULL row never matches
    assert kf.allowed_for(col, valid, kf.RANGE, lo, hi, 0, mask).tolist() == [1, 0, 0, 0, 0, 0, 1, 0]
    assert not kf.allowed_for(col, None, kf.RANGE, lo, hi, 1).any()                                      # lo > hi: nothing, no error
    assert kf.allowed_for(col, None, kf.RANGE, lo, hi, 2).tolist() == (col == -1).tolist()
    assert kf.allowed_for(col, valid, kf.RANGE, lo, hi, 3).tolist() == valid.astype(bool).tolist()       # every valid row
    assert not kf.allowed_for(col, None, kf.RANGE, lo, hi, 4).any()                                      # widened, never truncated
    assert kf.allowed_for(col, None, kf.RANGE, lo, hi, 5).tolist() == (col >= 3).tolist()                # half open
    wide = col.astype(np.int64) + 2 ** 40
    assert kf.allowed_for(wide, None, kf.RANGE, lo, hi, 4).tolist() == (col >= 0).tolist()             # -1 + 2^40 lies below 2^40
    lims, vals = kf.sets_to_csr([[7, 3, 7], [], [5, 1, -2], [kf.INT64_MIN, kf.INT64_MAX, 0], [2 ** 32 + 3]])
    assert lims.tolist() == [0, 2, 2, 5, 8, 9] and vals[:2].tolist() == [3, 7] and vals[2:5].tolist() == [-2, 1, 5]
    assert kf.allowed_for(col, None, kf.IN, lims, vals, 0).tolist() == [1, 0, 1, 1, 0, 1, 0, 1]
    assert kf.allowed_for(col, valid, kf.IN, lims, vals, 0, mask).tolist() == [1, 0, 0, 1, 0, 0, 0, 0]
    assert not kf.allowed_for(col, None, kf.IN, lims, vals, 1).any()                                     # an empty set
    assert not kf.allowed_for(col, None, kf.IN, lims, vals, 2).any()                                     # absent on both sides
    assert kf.allowed_for(col, None, kf.IN, lims, vals, 3).tolist() == (col == 0).tolist()
    assert not kf.allowed_for(col, None, kf.IN, lims, vals, 4).any()                                     # 2^32 + 3 is not 3
    ends = np.array([kf.INT64_MIN, kf.INT64_MAX, 0, -1], np.int64)
    assert kf.allowed_for(ends, None, kf.IN, lims, vals, 3).tolist() == [1, 1, 1, 0]
    with pytest.raises(OverflowError):
        kf.allowed_for(col, None, kf.RANGE, [0], [2 ** 63], 0)
    with pytest.raises(TypeError):
        kf.allowed_for(np.zeros(3, np.float32), None, kf.EQ, [0], None, 0)
    with pytest.raises(ValueError):
        kf.allowed_for(col, None, 3, [0], [0], 0)
    with pytest.raises(ValueError):
        kf.sets_to_csr([range(1025)])
    assert kf.sets_to_csr([range(1024)])[0].tolist() == [0, 1024]


def test_restatement_feeds_the_masked_restatement():
    """capped first, then filtered, at the unmasked positions"""
    cand = np.array([5, 1, 4, 2, 0, 3], np.uint32)
    col = np.array([9, 8, 10, 9, 8, 11], np.int64)
    valid = np.array([1, 1, 1, 1, 1, 0], np.uint8)          # row 5 is NULL
    data = np.arange(6, dtype=np.float32).reshape(6, 1)
    a = kf.allowed_for(col, valid, kf.RANGE, [9], [11], 0)          # rows 0, 2, 3 (5 is NULL)
    rows, pos = mask_ref.considered(cand, a, max_candidates=4)
    assert rows.tolist() == [2] and pos.tolist() == [3]
    rows, pos = mask_ref.considered(cand, a)
    assert rows.tolist() == [2, 0, 3] and pos.tolist() == [3, 4, 5]
    r, d2, nc, ncons = mask_ref.masked_topk(cand, a, data, np.zeros(1, np.float32), 2)
    assert r.tolist() == [0, 2] and d2.tolist() == [0.0, 4.0] and nc == 6 and ncons == 3
    lims, vals = kf.sets_to_csr([[8, 11]])
    r, out, nw, nc = mask_ref.masked_range(cand, kf.allowed_for(col, valid, kf.IN, lims, vals, 0), data, np.zeros(1, np.float32), 2.5)
    assert r.tolist() == [1] and nw == 1 and nc == 6
    shared = np.array([1, 0, 1, 1, 1, 1], bool)
    r, _, nw, _ = mask_ref.masked_range(cand, kf.allowed_for(col, valid, kf.IN, lims, vals, 0, shared), data, np.zeros(1, np.float32), 10.0)
    assert r.tolist() == [4] and nw == 1


def test_filtered_symbols_and_constants_exported_bound_and_in_sys_rs(lib):
    from pq_vector_amd import _ffi
    import pq_vector_amd as pqv
    hdr = open(os.path.join(ROOT, "include", "pqv.h")).read()
    sys_rs = open(os.path.join(ROOT, "bindings", "rust", "src", "sys.rs")).read()
    raw = C.CDLL(_ffi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _ffi.SIGNATURES
        assert getattr(lib, name).argtypes == _ffi.SIGNATURES[name][1]
        assert re.search(r"\b%s\s*\(" % name, hdr)
        assert re.search(r"pub fn %s\(" % name, sys_rs)
    for name, value in NEW_CONSTANTS.items():
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), hdr), name
        assert getattr(_ffi, name) == value and getattr(pqv, name) == value and name in pqv.__all__
        assert re.search(r"pub const %s: \w+ = %d;" % (name, value), sys_rs), name
    assert kf.SET_MAX == _ffi.PQV_KEY_SET_MAX and (kf.EQ, kf.RANGE, kf.IN) == (0, 1, 2)
    # the keyed twins' arities: the descriptor stands where qkeys stands
    for twin in ("pqv_topk_keyed", "pqv_topk_keyed_device", "pqv_range_search_keyed"):
        assert len(_ffi.SIGNATURES[twin.replace("keyed", "filtered")][1]) == len(_ffi.SIGNATURES[twin][1])
    assert C.sizeof(_ffi.KeyFilter) == 24 and _ffi.KeyFilter.a.offset == 8 and _ffi.KeyFilter.b.offset == 16
    assert "} pqv_key_filter;" in hdr and "pub struct PqvKeyFilter" in sys_rs
    for f, needle in (("bindings/rust/src/lib.rs", "pub enum KeyFilter"), ("bindings/rust/src/lib.rs", "pub fn topk_filtered"),
                      ("pq-vector_amd/host/pqv.hpp", "class KeyFilter")):
        assert needle in open(os.path.join(ROOT, f)).read(), (f, needle)
    assert lib.pqv_abi_version() == 101


def test_filtered_c_abi_validates_the_descriptor_before_device_use(lib):
    from pq_vector_amd import _ffi
    inv = _ffi.PQV_ERR_INVALID
    fake = C.c_void_p(8)         # never dereferenced: the descriptor's checks and the NULL checks come first
    nq = 2
    q = (C.c_float * (4 * nq))()
    rows, dist = (C.c_uint32 * (2 * nq))(), (C.c_float * (2 * nq))()
    lims_o, rr, dd = _ffi.u64p(), _ffi.u32p(), _ffi.f32p()

    def topk(s, keys, f):
        return lib.pqv_topk_filtered(s, keys, f, None, q, nq, 4, 2, 1, 0, 0, 1, rows, dist, None, None)

    def device(s, keys, f):
        return lib.pqv_topk_filtered_device(s, keys, f, None, None, nq, 2, 1, 0, 0, 1, None, None, None, None, None, None)

    def rng(s, keys, f):
        return lib.pqv_range_search_filtered(s, keys, f, None, q, nq, 4, 1.0, 1, 0, 0, 0, 1, C.byref(lims_o), C.byref(rr), C.byref(dd), None, None)

    def flt(kind, a, b):
        return C.byref(_ffi.KeyFilter(kind, 0, C.cast(a, C.c_void_p) if a is not None else None,
                                      C.cast(b, C.c_void_p) if b is not None else None))

    def err(rc, text):
        assert rc == inv and text in lib.pqv_last_error(), (rc, lib.pqv_last_error())

    i64 = lambda *v: (C.c_int64 * len(v))(*v)
    u64 = lambda *v: (C.c_uint64 * len(v))(*v)
    big = i64(*range(1025))
    for call, host in ((topk, True), (device, False), (rng, True)):
        # the descriptor first, in the header's order -- with NULL handles, which come only behind it
        err(call(None, None, None), b"filter must not be NULL")
        err(call(None, None, flt(3, i64(1, 2), None)), b"unknown key filter kind 3")
        err(call(None, None, flt(0xFFFFFFFF, None, None)), b"unknown key filter kind 4294967295")
        err(call(None, None, flt(_ffi.PQV_KEY_EQ, None, None)), b"query keys must not be NULL")
        err(call(None, None, flt(_ffi.PQV_KEY_RANGE, None, i64(1, 2))), b"query keys must not be NULL")
        err(call(None, None, flt(_ffi.PQV_KEY_RANGE, i64(1, 2), None)), b"query keys must not be NULL")
        err(call(None, None, flt(_ffi.PQV_KEY_IN, u64(0, 1, 2), None)), b"query keys must not be NULL")
        err(call(None, None, flt(_ffi.PQV_KEY_IN, None, i64(1, 2))), b"query keys must not be NULL")
        if host:
            err(call(None, None, flt(_ffi.PQV_KEY_IN, u64(1, 1, 2), i64(1, 2))), b"query key sets must start at 0 and not decrease")
            err(call(None, None, flt(_ffi.PQV_KEY_IN, u64(0, 2, 1), i64(1, 2))), b"query key sets must start at 0 and not decrease")
            # (a decrease is reported ahead of an oversized set, an oversized set ahead of an unsorted one)
            err(call(None, None, flt(_ffi.PQV_KEY_IN, u64(0, 1025, 1024), big)), b"query key sets must start at 0 and not decrease")
            err(call(None, None, flt(_ffi.PQV_KEY_IN, u64(0, 0, 1025), big)), b"a query key set takes at most 1024 values")
            err(call(None, None, flt(_ffi.PQV_KEY_IN, u64(0, 2, 1027), i64(5, 5, *range(1025)))), b"a query key set takes at most 1024 values")
            err(call(None, None, flt(_ffi.PQV_KEY_IN, u64(0, 2, 4), i64(1, 2, 4, 4))), b"query key sets must be strictly ascending")
            err(call(None, None, flt(_ffi.PQV_KEY_IN, u64(0, 2, 4), i64(2, 1, 3, 4))), b"query key sets must be strictly ascending")
        # ... then the keyed calls' own, in their order
        for good in (flt(_ffi.PQV_KEY_EQ, i64(1, 2), None), flt(_ffi.PQV_KEY_RANGE, i64(1, 2), i64(0, 9)),
                     flt(_ffi.PQV_KEY_IN, u64(0, 1024, 1024), big), flt(_ffi.PQV_KEY_IN, u64(0, 0, 0), i64(0)),
                     flt(_ffi.PQV_KEY_IN, u64(0, 1, 3), i64(7, kf.INT64_MIN, kf.INT64_MAX))):
            err(call(None, fake, good), b"searcher must not be NULL")
            err(call(fake, None, good), b"row keys must not be NULL")
    assert not lims_o and not rr and not dd


class _FakeCorpus:
    rows = 6


def test_python_sets_are_sorted_deduplicated_and_capped():
    from pq_vector_amd import api
    lims, vals = api.key_sets_to_csr([[5, 1, 5, 3], (), np.array([2, 2, 2], np.int32), {kf.INT64_MAX, kf.INT64_MIN, 0}, range(1024),
                                      list(range(1024)) * 2], 6)
    assert lims.dtype == np.uint64 and vals.dtype == np.int64 and vals.flags.c_contiguous
    assert lims.tolist() == [0, 3, 3, 4, 7, 1031, 2055]
    assert vals[:3].tolist() == [1, 3, 5] and vals[3] == 2 and vals[4:7].tolist() == [kf.INT64_MIN, 0, kf.INT64_MAX]
    assert vals[7:1031].tolist() == list(range(1024)) and vals[1031:].tolist() == list(range(1024))
    ref_lims, ref_vals = kf.sets_to_csr([[5, 1, 5, 3], (), [2, 2, 2], {kf.INT64_MAX, kf.INT64_MIN, 0}, range(1024), list(range(1024)) * 2])
    assert (lims == ref_lims).all() and (vals == ref_vals).all()
    lims, vals = api.key_sets_to_csr([[], []], 2)
    assert lims.tolist() == [0, 0, 0] and vals.size >= 1            # (a readable address, never read)
    with pytest.raises(ValueError, match="at most 1024 values"):
        api.key_sets_to_csr([[1], range(1025)], 2)
    with pytest.raises(api.PqvError, match="1 query key sets for 2 queries"):
        api.key_sets_to_csr([[1]], 2)
    with pytest.raises(api.PqvError, match="query keys must be integers"):
        api.key_sets_to_csr([[1.5]], 1)
    with pytest.raises(api.PqvError, match="query keys must fit int64"):
        api.key_sets_to_csr([np.array([2 ** 63], np.uint64)], 1)


def test_python_filter_keywords_are_checked_before_device_use():
    import pq_vector_amd as pqv
    s = object.__new__(pqv.Searcher)       # no device here: the checks must come before the library is asked
    s._h, s.dim, s.n_clusters, s._corpus, s._columns = None, 4, 2, _FakeCorpus(), {}
    q = np.zeros((2, 4), np.float32)
    closed = pqv.RowKeys(None, s)
    fake = pqv.RowKeys(8, s)               # (a handle that is never handed to the library)
    host = (lambda **kw: s.topk(q, 2, 1, **kw), lambda **kw: s.range_search(q, 1.0, 1, **kw))
    dev = (lambda **kw: s.topk_device(8, 2, 2, 1, 8, 8, **kw),)
    for call in host + dev:
        rg = (8, 16) if call in dev else ([1, 2], [3, 4])
        st = (8, 16) if call in dev else [[1], [2, 3]]
        for kw in (dict(query_keys=rg[0], query_key_ranges=rg), dict(query_keys=rg[0], query_key_sets=st),
                   dict(query_key_ranges=rg, query_key_sets=st), dict(query_keys=rg[0], query_key_ranges=rg, query_key_sets=st)):
            with pytest.raises(pqv.PqvError, match="mutually exclusive"):
                call(keys=fake, **kw)
        for kw in (dict(query_key_ranges=rg), dict(query_key_sets=st)):
            with pytest.raises(pqv.PqvError, match="keys must be a RowKeys"):          # the new keywords need keys=
                call(keys=None, **kw)
            with pytest.raises(pqv.PqvError, match="row keys must not be NULL"):
                call(keys=closed, **kw)
        with pytest.raises(pqv.PqvError, match="must be a pair"):
            call(keys=fake, query_key_ranges=5)
    for call in host:
        with pytest.raises(pqv.PqvError, match="1 query keys for 2 queries"):
            call(keys=fake, query_key_ranges=([1], [2, 3]))
        with pytest.raises(pqv.PqvError, match="3 query key sets for 2 queries"):
            call(keys=fake, query_key_sets=[[1], [2], [3]])
        with pytest.raises(ValueError, match="at most 1024 values"):
            call(keys=fake, query_key_sets=[[1], range(2000)])
        with pytest.raises(pqv.PqvError, match="query keys must be integers"):
            call(keys=fake, query_key_ranges=([1.0, 2.0], [3, 4]))
    with pytest.raises(pqv.PqvError, match="must be a pair"):
        dev[0](keys=fake, query_key_sets=[[1], [2], [3]])
    assert issubclass(pqv.TableSearcher, pqv.Searcher)          # (the keywords are the base class's: a table searcher takes them as they are)
    fake._h = None
