"""Expanding filtered top-k (pqv.h: pqv_topk_expand), host side: the numpy restatement of the depth rule (tests/expand_ref.py)
on hand-made lists and on the oracle-built shapes the GPU tests use, the ABI surface, and every check the C ABI and the Python
wrapper make before any device use, in the contract's order."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import expand_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pqv_topk_expand", "pqv_topk_expand_device")


@pytest.fixture(scope="module")
def lib():
    from pq_vector_amd import _ffi
    return _ffi.lib()


def test_restatement_on_hand_made_lists(oracle):
    # three lists around the centroids 0, 10, 20 on a line: a query at 1 probes them in the order 0, 1, 2
    cents = np.array([[0.0], [10.0], [20.0]], np.float32)
    lists = [np.array([0, 1, 2], np.uint32), np.array([3, 4], np.uint32), np.array([5, 6, 7, 8], np.uint32)]
    oidx = oracle.index_from_parts(1, cents, lists)
    q = np.array([1.0], np.float32)
    assert expand_ref.probe_order(oidx, q, 3).tolist() == [0, 1, 2]
    assert expand_ref.probe_order(oidx, np.array([19.0], np.float32), 2).tolist() == [2, 1]
    M = np.array([1, 0, 0, 0, 1, 1, 1, 1, 0], bool)
    assert expand_ref.prefix_counts(oidx, lists, M, q, 3).tolist() == [1, 2, 5]
    used = lambda k, np0, mx: expand_ref.nprobe_used(oidx, lists, M, q, k, np0, mx)
    assert used(1, 1, 3) == 1 and used(2, 1, 3) == 2 and used(3, 1, 3) == 3 and used(5, 1, 3) == 3
    assert used(6, 1, 3) == 3                      # never satisfied: P
    assert used(1, 2, 3) == 2                      # never below p0
    assert used(3, 1, 2) == 2                      # capped by max_nprobe
    assert used(3, 1, 1000) == 3 and used(1, 7, 1000) == 3        # both clamped to the 3 lists
    assert used(1, 1, 1) == 1 and used(9, 2, 2) == 2              # max_nprobe == nprobe: the twin call
    with pytest.raises(ValueError):
        used(1, 2, 1)
    assert [expand_ref.n_candidates(oidx, lists, q, u) for u in (1, 2, 3)] == [3, 5, 9]
    per_query = np.stack([M, np.zeros(9, bool)])
    assert expand_ref.used_for_batch(oidx, lists, per_query, np.stack([q, q]), 2, 1, 3).tolist() == [2, 3]
    assert expand_ref.used_for_batch(oidx, lists, M, np.stack([q, q]), 2, 1, 3).tolist() == [2, 2]


def test_restatement_on_the_first_gpu_shape(oracle):
    """the data recipe of tests/test_gpu_expand.py, shape 1: the depths the GPU test's premises rest on"""
    rng = np.random.default_rng(139)
    data = rng.random((4096, 128), dtype=np.float32)
    queries = rng.random((16, 128), dtype=np.float32)
    built = oracle.build_index(data, n_clusters=16, max_iters=5, workers=1)
    lists = built.lists()
    m64, m8 = rng.random(4096) < 1 / 64, rng.random(4096) < 1 / 8
    lens = sorted(len(l) for l in lists)
    assert len(lists) == 16 and lens[0] >= 1 and lens[-1] > 512 and any(int(o) % 64 for o in built.list_off[1:-1])
    a = expand_ref.used_for_batch(built, lists, m64, queries, 10, 1, 16)
    b = expand_ref.used_for_batch(built, lists, m8, queries, 100, 1, 16)
    for u in (a, b):
        assert len(set(u.tolist())) >= 3 and (u == 1).any(), u.tolist()
    # monotone in k, never below p0, never beyond P
    for k in (1, 10, 100):
        lo = expand_ref.used_for_batch(built, lists, m8, queries, k, 2, 5)
        hi = expand_ref.used_for_batch(built, lists, m8, queries, k + 50, 2, 5)
        assert (lo >= 2).all() and (hi <= 5).all() and (lo <= hi).all()


def test_symbols_exported_bound_and_in_sys_rs(lib):
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
    # the filtered twins' arities: max_nprobe stands where max_candidates stands, nprobe_used is one more pointer
    assert len(_ffi.SIGNATURES["pqv_topk_expand"][1]) == len(_ffi.SIGNATURES["pqv_topk_filtered"][1]) + 1
    assert len(_ffi.SIGNATURES["pqv_topk_expand_device"][1]) == len(_ffi.SIGNATURES["pqv_topk_filtered_device"][1]) + 1
    assert _ffi.SIGNATURES["pqv_topk_expand"][1][9] is C.c_uint32 and _ffi.SIGNATURES["pqv_topk_filtered"][1][9] is C.c_uint64
    assert "pub fn topk_expand" in open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    assert lib.pqv_abi_version() == 101


def test_c_abi_checks_before_device_use_in_the_contracts_order(lib):
    from pq_vector_amd import _ffi
    inv = _ffi.PQV_ERR_INVALID
    fake = C.c_void_p(8)         # never dereferenced: every check below comes before a handle is read
    nq = 2
    q = (C.c_float * (4 * nq))()
    rows, dist, used = (C.c_uint32 * (2 * nq))(), (C.c_float * (2 * nq))(), (C.c_uint32 * nq)()

    def host(s, keys, f, mask, nprobe=1, max_nprobe=4):
        return lib.pqv_topk_expand(s, keys, f, mask, q, nq, 4, 2, nprobe, max_nprobe, 0, 1, rows, dist, None, None, used)

    def device(s, keys, f, mask, nprobe=1, max_nprobe=4):
        return lib.pqv_topk_expand_device(s, keys, f, mask, None, nq, 2, nprobe, max_nprobe, 0, 1, None, None, None, None, None, None, None)

    def flt(kind, a, b):
        return C.byref(_ffi.KeyFilter(kind, 0, C.cast(a, C.c_void_p) if a is not None else None,
                                      C.cast(b, C.c_void_p) if b is not None else None))

    def err(rc, text):
        assert rc == inv and text in lib.pqv_last_error(), (rc, lib.pqv_last_error())

    i64 = lambda *v: (C.c_int64 * len(v))(*v)
    u64 = lambda *v: (C.c_uint64 * len(v))(*v)
    big = i64(*range(1025))
    good = flt(_ffi.PQV_KEY_EQ, i64(1, 2), None)
    for call, is_host in ((host, True), (device, False)):
        # 1: the searcher, whatever else is wrong
        err(call(None, None, None, None), b"searcher must not be NULL")
        err(call(None, fake, None, fake, 3, 1), b"searcher must not be NULL")
        err(call(None, None, flt(9, None, None), None), b"searcher must not be NULL")
        # 2: neither a mask nor keys -- ahead of a filter without keys
        err(call(fake, None, None, None), b"pqv_topk_expand needs a row mask or row keys")
        err(call(fake, None, good, None), b"pqv_topk_expand needs a row mask or row keys")
        err(call(fake, None, None, None, 3, 1), b"pqv_topk_expand needs a row mask or row keys")
        # 3: a filter without keys
        err(call(fake, None, good, fake), b"a key filter needs row keys")
        err(call(fake, None, flt(9, None, None), fake, 3, 1), b"a key filter needs row keys")
        # 4: keys without a filter
        err(call(fake, fake, None, None), b"filter must not be NULL")
        err(call(fake, fake, None, fake, 3, 1), b"filter must not be NULL")
        # 5: the descriptor, as the filtered host form checks it -- ahead of max_nprobe
        err(call(fake, fake, flt(3, i64(1, 2), None), None, 3, 1), b"unknown key filter kind 3")
        err(call(fake, fake, flt(_ffi.PQV_KEY_EQ, None, None), None, 3, 1), b"query keys must not be NULL")
        err(call(fake, fake, flt(_ffi.PQV_KEY_RANGE, i64(1, 2), None), None), b"query keys must not be NULL")
        err(call(fake, fake, flt(_ffi.PQV_KEY_IN, None, i64(1, 2)), fake), b"query keys must not be NULL")
        if is_host:
            err(call(fake, fake, flt(_ffi.PQV_KEY_IN, u64(1, 1, 2), i64(1, 2)), None, 3, 1), b"query key sets must start at 0 and not decrease")
            err(call(fake, fake, flt(_ffi.PQV_KEY_IN, u64(0, 0, 1025), big), None), b"a query key set takes at most 1024 values")
            err(call(fake, fake, flt(_ffi.PQV_KEY_IN, u64(0, 2, 4), i64(1, 2, 4, 4)), None, 3, 1), b"query key sets must be strictly ascending")
        # 6: max_nprobe -- ahead of everything that reads a handle
        for f in (good, flt(_ffi.PQV_KEY_RANGE, i64(1, 2), i64(0, 9)), flt(_ffi.PQV_KEY_IN, u64(0, 1, 3), i64(7, 8, 9))):
            err(call(fake, fake, f, None, 3, 2), b"max_nprobe must be >= nprobe")
            err(call(fake, fake, f, fake, 1, 0), b"max_nprobe must be >= nprobe")
        err(call(fake, None, None, fake, 5, 4), b"max_nprobe must be >= nprobe")


class _FakeCorpus:
    rows = 6


def test_python_wrapper_checks_before_device_use():
    import pq_vector_amd as pqv
    from pq_vector_amd import _ffi
    s = object.__new__(pqv.Searcher)       # no device here: the checks must come before the library is asked
    s._h, s.dim, s.n_clusters, s._corpus, s._columns = None, 4, 2, _FakeCorpus(), {}
    q = np.zeros((2, 4), np.float32)
    fake = pqv.RowKeys(8, s)
    try:
        with pytest.raises(pqv.PqvError, match="max_nprobe and max_candidates are mutually exclusive"):
            s.topk(q, 2, 1, max_candidates=5, max_nprobe=4, keys=fake, query_keys=[1, 2])
        with pytest.raises(pqv.PqvError, match="max_nprobe and max_candidates are mutually exclusive"):
            s.topk_device(8, 2, 2, 1, 8, 8, max_candidates=5, max_nprobe=4, keys=fake, query_keys=8)
        with pytest.raises(pqv.PqvError, match="mutually exclusive"):
            s.topk(q, 2, 1, max_nprobe=4, keys=fake, query_keys=[1, 2], query_key_sets=[[1], [2]])
        with pytest.raises(pqv.PqvError, match="1 query keys for 2 queries"):
            s.topk(q, 2, 1, max_nprobe=4, keys=fake, query_keys=[1])
    finally:
        fake._h = None
    # the builders: no filter is refused with the library's own text, a table builder takes no max_nprobe
    b = pqv.TopkBuilder(s, q[0]).k(2).nprobe(1).max_nprobe(4)
    with pytest.raises(pqv.PqvError, match="pqv_topk_expand needs a row mask or row keys") as e:
        b.search()
    assert e.value.code == _ffi.PQV_ERR_INVALID
    with pytest.raises(pqv.PqvError, match="max_nprobe must be > 0"):
        pqv.TopkBuilder(s, q[0]).max_nprobe(0)
    t = pqv.TableTopkBuilder(["a.parquet", "b.parquet"], q[0]).k(2).nprobe(1).max_nprobe(4)
    with pytest.raises(pqv.PqvError, match="pqv_topk_expand does not take table searchers") as e:
        t.search()
    assert e.value.code == _ffi.PQV_ERR_UNSUPPORTED
