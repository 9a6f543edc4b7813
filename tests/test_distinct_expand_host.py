"""Expanding distinct / grouped top-k (pqv.h: pqv_topk_distinct_expand, pqv_topk_grouped_expand), host side: the ABI surface, every
check the C ABI and the Python wrapper make before any device use in the contract's order, the numpy restatement of the depth rule
(tests/distinct_expand_ref.py) with its properties, a host model of the counting kernel's hash set against len(set(..)), and the
vacuity conditions of the fixtures tests/test_gpu_distinct_expand.py runs (tests/distinct_expand_cases.py), so that a dull fixture
fails here, without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import distinct_expand_cases as cases
import distinct_expand_ref as dref
import expand_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pqv_topk_distinct_expand", "pqv_topk_distinct_expand_device", "pqv_topk_grouped_expand", "pqv_topk_grouped_expand_device")


@pytest.fixture(scope="module")
def lib():
    from pq_vector_amd import _ffi
    return _ffi.lib()


def test_symbols_exported_bound_and_in_the_bindings(lib):
    from pq_vector_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "pqv.h")).read()
    sys_rs = open(os.path.join(ROOT, "bindings", "rust", "src", "sys.rs")).read()
    lib_rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    raw = C.CDLL(_ffi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _ffi.SIGNATURES
        assert getattr(lib, name).argtypes == _ffi.SIGNATURES[name][1]
        assert re.search(r"\b%s\s*\(" % name, hdr)
        assert re.search(r"pub fn %s\(" % name, sys_rs)
        # the filtered twins' arities: max_nprobe (u32) stands where max_candidates (u64) stands, nprobe_used is one more pointer
        twin = name.replace("_expand", "_filtered")
        args, targs = _ffi.SIGNATURES[name][1], _ffi.SIGNATURES[twin][1]
        assert len(args) == len(targs) + 1
        at = [i for i, t in enumerate(targs) if t is C.c_uint64]
        assert len(at) == 1 and args[at[0]] is C.c_uint32
        # ... and the same number of parameters in the header and in sys.rs
        decl = re.search(r"\bint %s\s*\(([^;]*)\);" % name, hdr).group(1)
        assert decl.count(",") + 1 == len(args)
        rs = re.search(r"pub fn %s\(([^;]*)\) -> c_int;" % name, sys_rs).group(1)
        assert rs.count(":") == len(args)
    assert "pub fn topk_distinct_expand" in lib_rs and "pub fn topk_grouped_expand" in lib_rs
    for gone in ("probing further lists when fewer than k groups are found.  (", "out of scope     expansion (max_nprobe) with a group column",
                 "distinct / grouped expansion, range search"):
        assert gone not in hdr
    assert lib.pqv_abi_version() == 101


def test_c_abi_checks_before_device_use_in_the_contracts_order(lib):
    from pq_vector_amd import _ffi
    inv = _ffi.PQV_ERR_INVALID
    fake = C.c_void_p(8)         # never dereferenced: every check below comes before a handle is read
    nq = 2
    q = (C.c_float * (4 * nq))()
    rows, dist, used = (C.c_uint32 * (6 * nq))(), (C.c_float * (6 * nq))(), (C.c_uint32 * nq)()

    def d_host(s, g, fk, f, mask, k=2, m=None, nprobe=1, max_nprobe=4):
        return lib.pqv_topk_distinct_expand(s, g, fk, f, mask, q, nq, 4, k, nprobe, max_nprobe, 0, 1, rows, dist, None, None, None, used)

    def d_dev(s, g, fk, f, mask, k=2, m=None, nprobe=1, max_nprobe=4):
        return lib.pqv_topk_distinct_expand_device(s, g, fk, f, mask, None, nq, k, nprobe, max_nprobe, 0, 1, None, None, None, None, None,
                                                   None, None)

    def g_host(s, g, fk, f, mask, k=2, m=3, nprobe=1, max_nprobe=4):
        return lib.pqv_topk_grouped_expand(s, g, fk, f, mask, q, nq, 4, k, m, nprobe, max_nprobe, 0, 1, rows, dist, None, None, None, None, used)

    def g_dev(s, g, fk, f, mask, k=2, m=3, nprobe=1, max_nprobe=4):
        return lib.pqv_topk_grouped_expand_device(s, g, fk, f, mask, None, nq, k, m, nprobe, max_nprobe, 0, 1, None, None, None, None, None,
                                                  None, None, None)

    def flt(kind, a, b):
        return C.byref(_ffi.KeyFilter(kind, 0, C.cast(a, C.c_void_p) if a is not None else None,
                                      C.cast(b, C.c_void_p) if b is not None else None))

    def err(rc, text):
        assert rc == inv and text in lib.pqv_last_error(), (rc, lib.pqv_last_error())

    i64 = lambda *v: (C.c_int64 * len(v))(*v)
    u64 = lambda *v: (C.c_uint64 * len(v))(*v)
    big = i64(*range(1025))
    good = flt(_ffi.PQV_KEY_EQ, i64(1, 2), None)
    bad_kind = flt(9, None, None)
    for call, is_host, grouped in ((d_host, True, False), (d_dev, False, False), (g_host, True, True), (g_dev, False, True)):
        # 1: the searcher, whatever else is wrong
        err(call(None, None, None, None, None), b"searcher must not be NULL")
        err(call(None, fake, None, bad_kind, fake, k=0, m=0, nprobe=3, max_nprobe=1), b"searcher must not be NULL")
        # 2: the group column, ahead of the filter pair
        err(call(fake, None, None, good, None), b"row keys must not be NULL")
        err(call(fake, None, fake, None, None, k=0, m=0, nprobe=3, max_nprobe=1), b"row keys must not be NULL")
        # 3: a filter without its column
        err(call(fake, fake, None, good, fake), b"a key filter needs row keys")
        err(call(fake, fake, None, bad_kind, None, k=0, m=0, nprobe=3, max_nprobe=1), b"a key filter needs row keys")
        # 4: a filter column without a filter
        err(call(fake, fake, fake, None, None), b"filter must not be NULL")
        err(call(fake, fake, fake, None, fake, k=0, m=0, nprobe=3, max_nprobe=1), b"filter must not be NULL")
        # 5: the descriptor, as pqv_topk_filtered checks it -- ahead of max_nprobe, k and group_size
        err(call(fake, fake, fake, flt(3, i64(1, 2), None), None, k=0, m=0, nprobe=3, max_nprobe=1), b"unknown key filter kind 3")
        err(call(fake, fake, fake, flt(_ffi.PQV_KEY_EQ, None, None), None, nprobe=3, max_nprobe=1), b"query keys must not be NULL")
        err(call(fake, fake, fake, flt(_ffi.PQV_KEY_RANGE, i64(1, 2), None), None, k=0), b"query keys must not be NULL")
        err(call(fake, fake, fake, flt(_ffi.PQV_KEY_IN, None, i64(1, 2)), fake, m=0), b"query keys must not be NULL")
        if is_host:
            err(call(fake, fake, fake, flt(_ffi.PQV_KEY_IN, u64(1, 1, 2), i64(1, 2)), None, nprobe=3, max_nprobe=1),
                b"query key sets must start at 0 and not decrease")
            err(call(fake, fake, fake, flt(_ffi.PQV_KEY_IN, u64(0, 0, 1025), big), None, k=0), b"a query key set takes at most 1024 values")
            err(call(fake, fake, fake, flt(_ffi.PQV_KEY_IN, u64(0, 2, 4), i64(1, 2, 4, 4)), None, m=0), b"query key sets must be strictly ascending")
        # 6: max_nprobe -- ahead of k, group_size and everything that reads a handle; with and without a filter
        for fk, f in ((fake, good), (fake, flt(_ffi.PQV_KEY_RANGE, i64(1, 2), i64(0, 9))), (fake, flt(_ffi.PQV_KEY_IN, u64(0, 1, 3), i64(7, 8, 9))),
                      (None, None)):
            err(call(fake, fake, fk, f, None, k=0, m=0, nprobe=3, max_nprobe=2), b"max_nprobe must be >= nprobe")
            err(call(fake, fake, fk, f, fake, nprobe=1, max_nprobe=0), b"max_nprobe must be >= nprobe")
            # 7: k, ahead of group_size
            err(call(fake, fake, fk, f, fake, k=0, m=0), b"k must be > 0")
            # 8: group_size
            if grouped:
                err(call(fake, fake, fk, f, fake, k=2, m=0), b"group_size must be > 0")


class _FakeCorpus:
    rows = 6


def test_python_wrapper_checks_before_device_use():
    import pq_vector_amd as pqv
    from pq_vector_amd import _ffi
    s = object.__new__(pqv.Searcher)       # no device here: the checks must come before the library is asked
    s._h, s.dim, s.n_clusters, s._corpus, s._columns = None, 4, 2, _FakeCorpus(), {}
    q = np.zeros((2, 4), np.float32)
    fake = pqv.RowKeys(8, s)
    text = "max_nprobe and max_candidates are mutually exclusive"
    try:
        with pytest.raises(pqv.PqvError, match=text):
            s.topk_distinct(q, 2, 1, fake, max_candidates=5, max_nprobe=4)
        with pytest.raises(pqv.PqvError, match=text):
            s.topk_grouped(q, 2, 3, 1, fake, max_candidates=5, max_nprobe=4, filter_keys=fake, query_keys=[1, 2])
        with pytest.raises(pqv.PqvError, match=text):
            s.topk_distinct_device(8, 2, 2, 1, fake, 8, 8, max_candidates=5, max_nprobe=4)
        with pytest.raises(pqv.PqvError, match=text):
            s.topk_grouped_device(8, 2, 2, 3, 1, fake, 8, 8, max_candidates=5, max_nprobe=4, filter_keys=fake, query_keys=8)
        with pytest.raises(pqv.PqvError, match="query_keys needs filter_keys="):
            s.topk_distinct(q, 2, 1, fake, max_nprobe=4, query_keys=[1, 2])
        with pytest.raises(pqv.PqvError, match="1 query keys for 2 queries"):
            s.topk_distinct(q, 2, 1, fake, max_nprobe=4, filter_keys=fake, query_keys=[1])
        with pytest.raises(pqv.PqvError, match="keys must be a RowKeys"):
            s.topk_distinct(q, 2, 1, 8, max_nprobe=4)
    finally:
        fake._h = None
    # the builders: max_nprobe with neither where() nor distinct_on() keeps its error; a table builder takes no max_nprobe
    with pytest.raises(pqv.PqvError, match="pqv_topk_expand needs a row mask or row keys") as e:
        pqv.TopkBuilder(s, q[0]).k(2).nprobe(1).max_nprobe(4).search()
    assert e.value.code == _ffi.PQV_ERR_INVALID
    with pytest.raises(pqv.PqvError, match="group_size\\(\\) needs distinct_on"):
        pqv.TopkBuilder(s, q[0]).k(2).nprobe(1).max_nprobe(4).group_size(3).search()
    t = pqv.TableTopkBuilder(["a.parquet", "b.parquet"], q[0]).k(2).nprobe(1).distinct_on("doc").max_nprobe(4)
    with pytest.raises(pqv.PqvError, match="pqv_topk_expand does not take table searchers") as e:
        t.search()
    assert e.value.code == _ffi.PQV_ERR_UNSUPPORTED


def test_restatement_on_hand_made_lists(oracle):
    # three lists around the centroids 0, 10, 20 on a line: a query at 1 probes them in the order 0, 1, 2
    cents = np.array([[0.0], [10.0], [20.0]], np.float32)
    lists = [np.array([0, 1, 2], np.uint32), np.array([3, 4], np.uint32), np.array([5, 6, 7, 8], np.uint32)]
    oidx = oracle.index_from_parts(1, cents, lists)
    q = np.array([1.0], np.float32)
    group = np.array([7, 7, 7, 7, -1, 9, 7, -1, 0], np.int64)
    assert dref.gcnt(oidx, lists, group, None, None, q, 3).tolist() == [1, 2, 4]          # 7 | 7, -1 | 9, 7, -1, 0
    valid = np.array([1, 1, 1, 1, 0, 1, 1, 1, 1], bool)
    assert dref.gcnt(oidx, lists, group, valid, None, q, 3).tolist() == [1, 1, 4]         # the NULL row never counts
    M = np.array([0, 0, 0, 1, 1, 1, 0, 0, 1], bool)
    assert dref.gcnt(oidx, lists, group, None, M, q, 3).tolist() == [0, 2, 4]
    assert dref.gcnt(oidx, lists, group, valid, M, np.array([19.0], np.float32), 2).tolist() == [2, 3]       # lists 2, 1
    used = lambda k, np0, mx, **kw: dref.nprobe_used(oidx, lists, group, kw.get("valid"), kw.get("M"), q, k, np0, mx)
    assert used(1, 1, 3) == 1 and used(2, 1, 3) == 2 and used(3, 1, 3) == 3 and used(4, 1, 3) == 3
    assert used(5, 1, 3) == 3                      # never satisfied: P
    assert used(1, 2, 3) == 2                      # a crossing before rank p0 - 1 still gives p0
    assert used(2, 1, 3, valid=valid) == 3         # the group seen at rank 0 and again at rank 1 counts once
    assert used(3, 1, 2) == 2                      # capped by max_nprobe
    assert used(3, 1, 1000) == 3 and used(1, 7, 1000) == 3        # both clamped to the 3 lists
    assert used(1, 1, 1) == 1 and used(9, 2, 2) == 2              # max_nprobe == nprobe: the twin call
    assert used(1, 1, 3, M=np.zeros(9, bool)) == 3                # nothing passes (an empty IN slice): P
    with pytest.raises(ValueError):
        used(1, 2, 1)
    # rows: 4 passing rows in the first two lists, but 2 groups
    assert dref.row_depth(oidx, lists, None, None, q, 4, 1, 3) == 2 and used(4, 1, 3) == 3
    per_query = np.stack([M, np.zeros(9, bool)])
    assert dref.used_for_batch(oidx, lists, group, None, per_query, np.stack([q, q]), 2, 1, 3).tolist() == [2, 3]
    assert dref.used_for_batch(oidx, lists, group, None, None, np.stack([q, q]), 2, 1, 3).tolist() == [2, 2]


@pytest.mark.parametrize("name", list(cases.MAIN))
def test_model_properties_and_vacuity_of_the_gpu_fixtures(oracle, name):
    """Seeds: base 20261, case i of MAIN 20262 + i (tests/distinct_expand_cases.py)."""
    c = cases.case(oracle, name)
    b = cases.base(oracle)
    assert cases.dull(c) == [], (name, c["used"].tolist(), c["rows_used"].tolist(), c["total"].tolist())
    k, p0, P = c["k"], c["nprobe"], c["max_nprobe"]
    M = c["M"]
    per_query = M is not None and np.asarray(M).ndim == 2
    prev = None
    for kk in (1, max(1, k // 2), k, k + 1, 3 * k):
        u = dref.used_for_batch(b["built"], b["lists"], c["group"], c["gvalid"], M, c["queries"], kk, p0, P)
        r = np.array([dref.row_depth(b["built"], b["lists"], c["gvalid"], M[i] if per_query else M, q, kk, p0, P)
                      for i, q in enumerate(c["queries"])])
        assert (u >= p0).all() and (u <= P).all()
        assert (u >= r).all()                                   # k groups need at least k rows
        assert prev is None or (u >= prev).all()                # monotone in k
        if kk == k:
            assert (u == c["used"]).all() and (r == c["rows_used"]).all()
        prev = u
    # the group column: 1 - 8 rows per group, scattered over more than one list
    _, sizes = np.unique(c["group"], return_counts=True)
    assert sizes.min() == 1 and sizes.max() == 8
    list_of = np.empty(cases.N, np.int64)
    for ci, l in enumerate(b["lists"]):
        list_of[np.asarray(l).astype(np.int64)] = ci
    spread = [len(set(list_of[c["group"] == g].tolist())) for g in np.unique(c["group"])[:200]]
    assert max(spread) >= 3 and np.mean(np.array(spread) > 1) > 0.25


def test_hash_set_model_counts_exactly():
    """the kernel's capacity, probe rule and empty marker (csrc/kernels.h: GROUP_SET_SLOTS, GROUP_SET_EMPTY, group_set_home)"""
    kh = open(os.path.join(ROOT, "pq-vector_amd", "csrc", "kernels.h")).read()
    assert "GROUP_SET_SLOTS = %d;" % dref.SET_SLOTS in kh and "GROUP_SET_EMPTY = ~0ull;" in kh
    assert "(v * 0x9E3779B97F4A7C15ull) >> 52" in kh
    assert dref.SET_EMPTY == np.array([-1], np.int64).view(np.uint64)[0]
    i64_min, i64_max = -(2 ** 63), 2 ** 63 - 1
    rng = np.random.default_rng(5)
    edge = [-1, 0, -1, i64_min, i64_max, 0, 1, -2, i64_min, -1]
    congruent = [7 + dref.SET_SLOTS * i for i in range(1100)]                      # equal modulo the table size
    inv = pow(0x9E3779B97F4A7C15, -1, 2 ** 64)
    same_home = [(((5 << 52) | i) * inv) % 2 ** 64 for i in range(1, 301)]         # 300 values whose home slot is 5
    assert {dref.set_home(v) for v in same_home} == {5}
    same_home = [v - 2 ** 64 if v >= 2 ** 63 else v for v in same_home]
    wrap = [(((4095 << 52) | i) * inv) % 2 ** 64 for i in range(1, 40)]            # ... and 39 at the last slot: the probe wraps
    wrap = [v - 2 ** 64 if v >= 2 ** 63 else v for v in wrap]
    rand = rng.integers(i64_min, i64_max, 200).tolist()
    for vals in (edge, congruent, same_home, wrap, edge + congruent + rand + congruent[::-1] + same_home + wrap + edge):
        s = dref.GroupSet()
        seen = set()
        for v in vals:
            new = s.insert(v)
            assert new == (v not in seen)
            seen.add(v)
            assert s.count == len(seen)
        assert s.count == len(set(vals))
        assert (-1 in seen) == s.marker and dref.SET_EMPTY not in [x for x in s.tab if x != dref.SET_EMPTY]
        assert sum(x != dref.SET_EMPTY for x in s.tab) == len(seen) - (1 if -1 in seen else 0)
    # the fullest the kernel's table gets: k - 1 counted values and 4 waves x 64 in flight
    s = dref.GroupSet()
    for v in range(1024 - 1 + 256):
        assert s.insert(v * 0x10001 - 77)
    assert s.count == 1279 and s.count < dref.SET_SLOTS // 3
    # congruent values do not crowd one slot: the multiplicative home spreads them (the probe stays short)
    s = dref.GroupSet()
    for v in congruent:
        s.insert(v)
    assert s.steps < 4 * len(congruent)
