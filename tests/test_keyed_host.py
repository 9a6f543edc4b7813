"""Per-query key filters, host side: the numpy restatement of M_q (tests/keyed_ref.py) through tests/mask_ref.py, the ABI
surface, and the argument validation that needs no device (NULL handles come first; the checks that read a real column or a
real searcher -- column type, row count, device, ownership -- need a device and are in tests/test_gpu_keyed.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import keyed_ref
import mask_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("pqv_row_keys_create", "pqv_row_keys_rows", "pqv_row_keys_dtype", "pqv_row_keys_free", "pqv_topk_keyed",
               "pqv_topk_keyed_device", "pqv_range_search_keyed")


@pytest.fixture(scope="module")
def lib():
    from pq_vector_amd import _ffi
    return _ffi.lib()


def test_restatement_is_the_contract():
    col = np.array([3, -1, 3, 7, -1, 3, 0, 7], np.int32)
    valid = np.array([1, 1, 0, 1, 1, 1, 1, 0], np.uint8)
    mask = np.array([1, 1, 1, 1, 0, 0, 1, 1], bool)
    assert keyed_ref.allowed_for(col, None, 3).tolist() == [1, 0, 1, 0, 0, 1, 0, 0]
    assert keyed_ref.allowed_for(col, valid, 3).tolist() == [1, 0, 0, 0, 0, 1, 0, 0]            # a NULL row never matches
    assert keyed_ref.allowed_for(col, valid, 3, mask).tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
    assert keyed_ref.allowed_for(col, valid, -1).tolist() == [0, 1, 0, 0, 1, 0, 0, 0]           # negative keys
    assert keyed_ref.allowed_for(col, valid, 7).tolist() == [0, 0, 0, 1, 0, 0, 0, 0]
    assert not keyed_ref.allowed_for(col, None, 5).any()                                        # a key no row has
    # an I32 value against 2**32 + value: widened, never truncated -- nothing matches
    for v in (3, -1, 0, 7):
        assert not keyed_ref.allowed_for(col, None, 2 ** 32 + v).any()
        assert keyed_ref.allowed_for(col.astype(np.int64) + 2 ** 32, None, 2 ** 32 + v).tolist() == (col == v).tolist()
    # the ends of i64
    wide = np.array([keyed_ref.INT64_MIN, keyed_ref.INT64_MAX, 0, -1, keyed_ref.INT64_MAX], np.int64)
    assert keyed_ref.allowed_for(wide, None, keyed_ref.INT64_MIN).tolist() == [1, 0, 0, 0, 0]
    assert keyed_ref.allowed_for(wide, None, keyed_ref.INT64_MAX).tolist() == [0, 1, 0, 0, 1]
    assert not keyed_ref.allowed_for(np.array([-1, 0, 2 ** 31 - 1, -2 ** 31], np.int32), None, keyed_ref.INT64_MIN).any()
    assert not keyed_ref.allowed_for(np.array([-1, 0, 2 ** 31 - 1, -2 ** 31], np.int32), None, keyed_ref.INT64_MAX).any()
    with pytest.raises(OverflowError):
        keyed_ref.allowed_for(wide, None, 2 ** 63)
    with pytest.raises(TypeError):
        keyed_ref.allowed_for(np.zeros(3, np.float32), None, 0)
    assert keyed_ref.group_by_key([5, 2, 5, -1]) == {5: [0, 2], 2: [1], -1: [3]}


def test_restatement_feeds_the_masked_restatement():
    """capped first, then keyed, at the unmasked positions"""
    cand = np.array([5, 1, 4, 2, 0, 3], np.uint32)
    col = np.array([9, 8, 9, 9, 8, 9], np.int64)            # rows 0, 2, 3, 5 carry key 9
    valid = np.array([1, 1, 1, 1, 1, 0], np.uint8)          # row 5 is NULL
    data = np.arange(6, dtype=np.float32).reshape(6, 1)
    a = keyed_ref.allowed_for(col, valid, 9)
    rows, pos = mask_ref.considered(cand, a, max_candidates=4)
    assert rows.tolist() == [2] and pos.tolist() == [3]
    rows, pos = mask_ref.considered(cand, a)
    assert rows.tolist() == [2, 0, 3] and pos.tolist() == [3, 4, 5]
    r, d2, nc, ncons = mask_ref.masked_topk(cand, a, data, np.zeros(1, np.float32), 2)
    assert r.tolist() == [0, 2] and d2.tolist() == [0.0, 4.0] and nc == 6 and ncons == 3
    r, out, nw, nc = mask_ref.masked_range(cand, keyed_ref.allowed_for(col, valid, 8), data, np.zeros(1, np.float32), 2.5)
    assert r.tolist() == [1] and nw == 1 and nc == 6
    r, _, nw, _ = mask_ref.masked_range(cand, keyed_ref.allowed_for(col, valid, 8, np.array([1, 0, 1, 1, 1, 1], bool)), data,
                                        np.zeros(1, np.float32), 10.0)
    assert r.tolist() == [4] and nw == 1


def test_keyed_symbols_exported_bound_and_in_sys_rs(lib):
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
    # the masked twins' arities plus keys, qkeys and the optional mask in place of the twin's mask: + 2
    assert len(_ffi.SIGNATURES["pqv_topk_keyed"][1]) == len(_ffi.SIGNATURES["pqv_topk_masked"][1]) + 2
    assert len(_ffi.SIGNATURES["pqv_topk_keyed_device"][1]) == len(_ffi.SIGNATURES["pqv_topk_masked_device"][1]) + 2
    assert len(_ffi.SIGNATURES["pqv_range_search_keyed"][1]) == len(_ffi.SIGNATURES["pqv_range_search_masked"][1]) + 2
    assert len(_ffi.SIGNATURES["pqv_row_keys_create"][1]) == 4
    assert "typedef struct pqv_row_keys pqv_row_keys;" in hdr and "pub struct PqvRowKeys" in sys_rs
    for f, needle in (("bindings/rust/src/lib.rs", "pub struct RowKeys"), ("bindings/rust/src/lib.rs", "impl Drop for RowKeys"),
                      ("pq-vector_amd/host/pqv.hpp", "class RowKeys")):
        assert needle in open(os.path.join(ROOT, f)).read(), (f, needle)
    assert lib.pqv_abi_version() == 101


def test_keyed_c_abi_validates_before_device_use(lib):
    from pq_vector_amd import _ffi
    inv = _ffi.PQV_ERR_INVALID
    h = C.c_void_p()
    fake = C.c_void_p(8)         # never dereferenced: the NULL checks come first
    assert lib.pqv_row_keys_create(None, fake, None, C.byref(h)) == inv and b"searcher must not be NULL" in lib.pqv_last_error()
    assert lib.pqv_row_keys_create(fake, fake, None, None) == inv and b"out must not be NULL" in lib.pqv_last_error()
    assert lib.pqv_row_keys_create(fake, None, None, C.byref(h)) == inv and b"column must not be NULL" in lib.pqv_last_error()
    assert not h.value
    q = (C.c_float * 4)()
    qk = (C.c_int64 * 1)(5)
    rows, dist = (C.c_uint32 * 2)(), (C.c_float * 2)()
    lims, rr, dd = _ffi.u64p(), _ffi.u32p(), _ffi.f32p()

    def topk(s, keys, qkeys):
        return lib.pqv_topk_keyed(s, keys, qkeys, None, q, 1, 4, 2, 1, 0, 0, 1, rows, dist, None, None)

    def device(s, keys, qkeys):
        return lib.pqv_topk_keyed_device(s, keys, qkeys, None, None, 1, 2, 1, 0, 0, 1, None, None, None, None, None, None)

    def rng(s, keys, qkeys):
        return lib.pqv_range_search_keyed(s, keys, qkeys, None, q, 1, 4, 1.0, 1, 0, 0, 0, 1, C.byref(lims), C.byref(rr), C.byref(dd), None, None)

    for call, host in ((topk, True), (device, False), (rng, True)):
        keys_arg = qk if host else fake
        assert call(None, fake, keys_arg) == inv and b"searcher must not be NULL" in lib.pqv_last_error()
        assert call(fake, None, keys_arg) == inv and b"row keys must not be NULL" in lib.pqv_last_error()
    # (query keys are checked behind the handles: with a real handle in tests/test_gpu_keyed.py)
    assert lib.pqv_row_keys_rows(None) == 0 and lib.pqv_row_keys_dtype(None) == -1
    lib.pqv_row_keys_free(None)


class _FakeCorpus:
    rows = 6


def test_python_keyed_arguments_are_checked_before_device_use():
    import pq_vector_amd as pqv
    assert pqv.RowKeys in (getattr(pqv, n) for n in pqv.__all__)
    s = object.__new__(pqv.Searcher)       # no device here: the checks must come before the library is asked
    s._h, s.dim, s.n_clusters, s._corpus, s._columns = None, 4, 2, _FakeCorpus(), {}
    q = np.zeros((2, 4), np.float32)
    with pytest.raises(pqv.PqvError, match="no column named 'tenant' is attached"):
        s.row_keys("tenant")
    with pytest.raises(pqv.PqvError, match="column must not be NULL"):
        s.row_keys(None)
    closed = pqv.RowKeys(None, s)
    assert closed.rows == 0 and closed.dtype == -1
    fake = pqv.RowKeys(8, s)               # (a handle that is never handed to the library)
    for call in (lambda **kw: s.topk(q, 2, 1, **kw), lambda **kw: s.range_search(q, 1.0, 1, **kw),
                 lambda **kw: s.topk_device(8, 2, 2, 1, 8, 8, **kw)):
        with pytest.raises(pqv.PqvError, match="row keys must not be NULL"):
            call(keys=closed, query_keys=[1, 2])
        with pytest.raises(pqv.PqvError, match="keys must be a RowKeys"):
            call(keys=None, query_keys=[1, 2])
        with pytest.raises(pqv.PqvError, match="query keys must not be NULL"):
            call(keys=fake, query_keys=None)
    fake._h = None

