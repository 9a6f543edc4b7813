"""Key partitions (pqv.h: pqv_key_partition, pqv_topk_partition), host side: the numpy restatement (tests/partition_ref.py) against
key_filter_ref / mask_ref run over the one-list index S1 of the contract's equivalence, the conditions on the GPU tests' inputs
(tests/partition_cases.py), the ABI surface, the validation order -- all of it before any device use -- and the Python wrapper's
argument handling."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import key_filter_ref as kf
import long_rows_cases as lrc
import mask_ref
import partition_cases as pc
import partition_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("pqv_key_partition_create", "pqv_key_partition_rows", "pqv_key_partition_n_keys", "pqv_key_partition_dtype",
               "pqv_key_partition_keys", "pqv_key_partition_free", "pqv_topk_partition", "pqv_topk_partition_device")


@pytest.fixture(scope="module")
def lib():
    from pq_vector_amd import _ffi
    return _ffi.lib()


def test_shapes_are_the_masked_tests_shapes():
    import test_gpu_mask
    assert set(pc.SHAPES) == set(test_gpu_mask.SHAPES)
    for name, c in test_gpu_mask.SHAPES.items():
        assert {k: pc.SHAPES[name][k] for k in c} == c, name
    assert set(pc.LONG_SHAPES) <= set(lrc.SHAPES)
    assert {lrc.SHAPES[n]["kind"] for n in pc.LONG_SHAPES} == {"l2", "dot", "cos"}


@pytest.mark.parametrize("name", list(pc.SHAPES))
def test_inputs_have_no_equal_distances_and_cover_the_layouts(name):
    c = pc.Case(name)
    c.assert_distinct()
    cols = c.columns
    assert cols["t3"][0].dtype == np.int32 and cols["t3"][1] is None and cols["t3"][0].min() < 0
    assert np.unique(cols["t3"][0], return_counts=True)[1].min() > 256          # runs longer than a block's turn
    assert cols["t64"][0].dtype == np.int64 and (cols["t64"][1] == 0).any()
    assert np.abs(cols["t64"][0]).min() > 2 ** 31 and cols["t64"][0].min() < 0 and len(np.unique(cols["t64"][0])) == 64
    assert cols["distinct"][0].dtype == np.int32 and len(np.unique(cols["distinct"][0])) == c.n and (cols["distinct"][1] == 0).any()
    v, cnt = np.unique(cols["skew"][0], return_counts=True)
    assert cnt.max() > 512 and (np.sort(cnt)[:-1] == 1).all()
    for col in cols:
        fl = c.filters(col)
        assert [f[1] for f in fl] == [kf.EQ, kf.RANGE, kf.IN]
        lims = fl[2][2]
        sizes = {lims[i + 1] - lims[i] for i in range(c.nq)}
        assert 0 in sizes and 1 in sizes and max(sizes) <= kf.SET_MAX
        assert any(a > b for a, b in zip(fl[1][2], fl[1][3])), "an inverted range"
        assert (kf.INT64_MIN, kf.INT64_MAX) in set(zip(fl[1][2], fl[1][3])), "the full range"
    assert {max(c.filters(col)[2][2][i + 1] - c.filters(col)[2][2][i] for i in range(c.nq)) for col in ("t64", "distinct", "skew")} == {1024}
    assert any(abs(v) > 2 ** 31 for v in c.filters("t3")[0][2]), "a query key outside i32 on the I32 column"


def test_seventy_queries_case():
    c = pc.Case("1500x30")
    assert c.nq == 70
    c.assert_distinct()


@pytest.mark.parametrize("name", pc.LONG_SHAPES)
def test_long_row_inputs_are_distinct(name, oracle):
    lrc.Case(name, oracle).assert_distinct()


def test_restatement_is_the_contract():
    col = np.array([3, -1, 3, 7, -1, 3, 0, 7, 3], np.int32)
    valid = np.array([1, 1, 0, 1, 1, 1, 1, 0, 1], np.uint8)
    indexed = [8, 0, 1, 2, 3, 4, 5, 6]                   # row 7 is in no list; row 2 and 7 have NULL keys
    rows, keys = pr.build(col, valid, indexed)
    assert rows.tolist() == [1, 4, 6, 0, 5, 8, 3] and keys.tolist() == [-1, -1, 0, 3, 3, 3, 7]
    v, c = pr.distinct(keys)
    assert v.tolist() == [-1, 0, 3, 7] and c.tolist() == [2, 1, 3, 1]
    assert pr.sequence(keys, kf.EQ, [3], None, 0).tolist() == [3, 4, 5]
    assert pr.sequence(keys, kf.EQ, [2 ** 32 + 3], None, 0).tolist() == []
    assert pr.sequence(keys, kf.RANGE, [0], [3], 0).tolist() == [2, 3, 4, 5]
    assert pr.sequence(keys, kf.RANGE, [3], [0], 0).tolist() == []
    assert pr.sequence(keys, kf.RANGE, [kf.INT64_MIN], [kf.INT64_MAX], 0).tolist() == list(range(7))
    assert pr.sequence(keys, kf.IN, [0, 3], [-1, 5, 7], 0).tolist() == [0, 1, 6]
    assert pr.sequence(keys, kf.IN, [0, 0], [], 0).tolist() == []
    # positions are the unmasked ones; order by (distance, position); slots past n_found are EMPTY / +inf
    d = np.array([5, 1, 9, 2, 1, 5, 0, 0, 4], np.float32)
    allow = np.ones(9, bool)
    allow[6] = False
    r, dd, nf, nc, considered = pr.topk(rows, keys, kf.RANGE, [-1], [3], 0, d, 4, allow=allow)
    assert (nf, nc, considered) == (4, 6, 5) and r.tolist() == [1, 4, 8, 0] and dd.tolist() == [1, 1, 4, 5]
    r, dd, nf, nc, _ = pr.topk(rows, keys, kf.EQ, [7], None, 0, d, 3)
    assert (nf, nc) == (1, 1) and r.tolist() == [3, pr.EMPTY, pr.EMPTY] and dd[0] == 2 and np.isinf(dd[1:]).all()
    # PQV_DOT orders signed distances
    assert pr.order_bits("dot", np.array([-2, -0.5, 0, 3], np.float32)).tolist() == sorted(pr.order_bits("dot", np.array([-2, -0.5, 0, 3], np.float32)).tolist())


@pytest.mark.parametrize("name", ["4096x128", "2048x32-seq"])
def test_restatement_equals_the_filtered_restatement_on_the_one_list_index(name):
    """S1: one list = all indexed rows ascending.  There key_filter_ref's M_q through mask_ref.masked_topk is the filtered call's
    restatement (nprobe = 1, no cap), and -- no two rows tie -- the partition's answer, EQ, RANGE and IN alike."""
    c = pc.Case(name)
    indexed = np.setdiff1d(np.arange(c.n), np.arange(5, c.n, 37))        # (as after a remove)
    shared = np.random.default_rng(9).random(c.n) < 0.5
    for col, (values, valid) in c.columns.items():
        part = c.partition(col, indexed)
        for flt in c.filters(col):
            _, kind, a, b = flt
            for allow in (None, shared):
                for k in (1, 10, 300):
                    rows, dist, nf, nc, _ = c.topk(part, flt, k, allow=allow)
                    for q in range(c.nq):
                        m_q = kf.allowed_for(values, valid, kind, a, b, q, allow)
                        er, ed, _, n_cons = mask_ref.masked_topk(indexed.astype(np.uint32), m_q, c.data, c.queries[q], k, metric=c.metric)
                        assert nf[q] == len(er) == min(k, n_cons) and (rows[q, :nf[q]] == er).all(), (col, flt[0], k, q)
                        assert (dist[q, :nf[q]].view(np.uint32) == ed.view(np.uint32)).all()
                        assert nc[q] == int(kf.allowed_for(values, valid, kind, a, b, q)[indexed].sum())


def test_partition_symbols_exported_bound_and_in_sys_rs(lib):
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
    # the filtered twins' arities less nprobe and max_candidates (and the device form's tie flags)
    assert len(_ffi.SIGNATURES["pqv_topk_partition"][1]) == len(_ffi.SIGNATURES["pqv_topk_filtered"][1]) - 2
    assert len(_ffi.SIGNATURES["pqv_topk_partition_device"][1]) == len(_ffi.SIGNATURES["pqv_topk_filtered_device"][1]) - 3
    assert "typedef struct pqv_key_partition pqv_key_partition;" in hdr and "pub struct PqvKeyPartition" in sys_rs
    for f, needle in (("bindings/rust/src/lib.rs", "pub struct KeyPartition"), ("bindings/rust/src/lib.rs", "pub fn topk_partition"),
                      ("pq-vector_amd/host/pqv.hpp", "class KeyPartition"), ("pq-vector_amd/csrc/Makefile", "kernels_partition.o"),
                      ("pq-vector_amd/csrc/kernels_all.hip", "kernels_partition.hip")):
        assert needle in open(os.path.join(ROOT, f)).read(), (f, needle)
    assert "KeyPartition" in pqv.__all__
    for m in ("key_partition", "topk_partition", "topk_partition_device"):
        assert callable(getattr(pqv.Searcher, m))
    assert lib.pqv_abi_version() == 101
    assert lib.pqv_key_partition_rows(None) == 0 and lib.pqv_key_partition_n_keys(None) == 0 and lib.pqv_key_partition_dtype(None) == -1
    lib.pqv_key_partition_free(None)


def test_partition_c_abi_validates_in_the_stated_order_before_device_use(lib):
    from pq_vector_amd import _ffi
    inv = _ffi.PQV_ERR_INVALID
    fake = C.c_void_p(8)                 # never dereferenced: every check below comes before a handle is read
    zeros = (C.c_uint8 * 4096)()         # a handle whose owner is nobody: read by the ownership check only
    other = C.cast(zeros, C.c_void_p)
    nq = 2
    q = (C.c_float * (4 * nq))()
    rows, dist = (C.c_uint32 * (2 * nq))(), (C.c_float * (2 * nq))()

    def host(s, part, f, k=2, mask=None):
        return lib.pqv_topk_partition(s, part, f, mask, q, nq, 4, k, 0, 1, rows, dist, None, None)

    def device(s, part, f, k=2, mask=None):
        return lib.pqv_topk_partition_device(s, part, f, mask, None, nq, k, 0, 1, None, None, None, None, None)

    def flt(kind, a, b):
        return C.byref(_ffi.KeyFilter(kind, 0, C.cast(a, C.c_void_p) if a is not None else None,
                                      C.cast(b, C.c_void_p) if b is not None else None))

    def err(rc, text, code=inv):
        assert rc == code and text in lib.pqv_last_error(), (rc, lib.pqv_last_error())

    i64 = lambda *v: (C.c_int64 * len(v))(*v)       # noqa: E731
    u64 = lambda *v: (C.c_uint64 * len(v))(*v)      # noqa: E731
    big = i64(*range(1025))
    good = flt(_ffi.PQV_KEY_EQ, i64(1, 2), None)
    for call, is_host in ((host, True), (device, False)):
        err(call(None, None, None), b"searcher must not be NULL")
        err(call(None, fake, good), b"searcher must not be NULL")
        err(call(fake, None, None), b"key partition must not be NULL")
        err(call(fake, None, good), b"key partition must not be NULL")
        err(call(fake, fake, None), b"filter must not be NULL")
        err(call(fake, fake, flt(3, i64(1, 2), None)), b"unknown key filter kind 3")
        err(call(fake, fake, flt(_ffi.PQV_KEY_EQ, None, None)), b"query keys must not be NULL")
        err(call(fake, fake, flt(_ffi.PQV_KEY_RANGE, i64(1, 2), None)), b"query keys must not be NULL")
        err(call(fake, fake, flt(_ffi.PQV_KEY_IN, None, i64(1, 2))), b"query keys must not be NULL")
        if is_host:
            err(call(fake, fake, flt(_ffi.PQV_KEY_IN, u64(1, 1, 2), i64(1, 2))), b"query key sets must start at 0 and not decrease")
            err(call(fake, fake, flt(_ffi.PQV_KEY_IN, u64(0, 2, 1), i64(1, 2))), b"query key sets must start at 0 and not decrease")
            err(call(fake, fake, flt(_ffi.PQV_KEY_IN, u64(0, 0, 1025), big)), b"a query key set takes at most 1024 values")
            err(call(fake, fake, flt(_ffi.PQV_KEY_IN, u64(0, 2, 4), i64(1, 2, 4, 4))), b"query key sets must be strictly ascending")
            # (the descriptor is checked ahead of k)
            err(call(fake, fake, flt(_ffi.PQV_KEY_IN, u64(0, 2, 4), i64(2, 1, 3, 4)), k=0), b"query key sets must be strictly ascending")
        for ok in (good, flt(_ffi.PQV_KEY_RANGE, i64(1, 2), i64(0, 9)), flt(_ffi.PQV_KEY_IN, u64(0, 1024, 1024), big)):
            err(call(fake, fake, ok, k=0), b"k must be > 0")
            err(call(fake, other, ok), b"key partition belongs to another searcher")
            err(call(fake, other, ok, k=1025), b"key partition belongs to another searcher")
    # creation: pqv_row_keys_create's texts in its order
    out = C.c_void_p(77)
    err(lib.pqv_key_partition_create(fake, fake, None, None), b"out must not be NULL")
    err(lib.pqv_key_partition_create(None, fake, None, C.byref(out)), b"searcher must not be NULL")
    assert out.value is None
    err(lib.pqv_key_partition_create(fake, None, None, C.byref(out)), b"column must not be NULL")
    err(lib.pqv_key_partition_keys(None, None, None, 4), b"key partition must not be NULL")


def test_python_wrappers_check_their_arguments_before_device_use():
    import pq_vector_amd as pqv
    s = object.__new__(pqv.Searcher)       # no device here: the checks must come before the library is asked
    s._columns = {}
    q = np.zeros((2, 4), np.float32)
    fake = pqv.KeyPartition(8, s)          # (a handle that is never handed to the library)
    try:
        with pytest.raises(pqv.PqvError, match="part must be a KeyPartition"):
            s.topk_partition(q, 2, pqv.RowKeys(None, s), query_keys=[1, 2])
        closed = pqv.KeyPartition(None, s)
        with pytest.raises(pqv.PqvError, match="key partition must not be NULL"):
            s.topk_partition(q, 2, closed, query_keys=[1, 2])
        with pytest.raises(pqv.PqvError, match="key partition must not be NULL"):
            closed.keys()
        assert closed.rows == 0 and closed.n_keys == 0 and closed.dtype == -1
        with pytest.raises(pqv.PqvError, match="query keys must not be NULL"):
            s.topk_partition(q, 2, fake)
        with pytest.raises(pqv.PqvError, match="mutually exclusive"):
            s.topk_partition(q, 2, fake, query_keys=[1, 2], query_key_sets=[[1], [2]])
        with pytest.raises(pqv.PqvError, match="1 query keys for 2 queries"):
            s.topk_partition(q, 2, fake, query_keys=[1])
        with pytest.raises(pqv.PqvError, match="1 query keys for 2 queries"):
            s.topk_partition(q, 2, fake, query_key_ranges=([1], [2, 3]))
        with pytest.raises(pqv.PqvError, match="must be a pair"):
            s.topk_partition(q, 2, fake, query_key_ranges=5)
        # a malformed IN set: the existing texts
        with pytest.raises(pqv.PqvError, match="3 query key sets for 2 queries"):
            s.topk_partition(q, 2, fake, query_key_sets=[[1], [2], [3]])
        with pytest.raises(ValueError, match="at most 1024 values"):
            s.topk_partition(q, 2, fake, query_key_sets=[[1], range(2000)])
        with pytest.raises(pqv.PqvError, match="query keys must be integers"):
            s.topk_partition(q, 2, fake, query_key_sets=[[1.5], [2]])
        with pytest.raises(pqv.PqvError, match="must be a pair"):
            s.topk_partition_device(8, 2, 2, fake, 8, 8, query_key_sets=[[1], [2], [3]])
        with pytest.raises(pqv.PqvError, match="no column named 'tenant'"):
            s.key_partition("tenant")
        with pytest.raises(pqv.PqvError, match="column must not be NULL"):
            s.key_partition(None)
    finally:
        fake._h = None
        s._h = None
