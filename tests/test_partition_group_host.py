"""Distinct / grouped top-k over a key partition (pqv.h: pqv_topk_partition_grouped), host side: the numpy restatement
(tests/partition_group_ref.py) against a brute-force statement of the contract, the conditions on the GPU tests' inputs
(tests/partition_group_cases.py), the ABI surface and the validation order -- all of it before any device use."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import key_filter_ref as kf
import partition_cases as pc
import partition_group_cases as pgc
import partition_group_ref as pgr
import partition_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pqv_topk_partition_grouped", "pqv_topk_partition_grouped_device")


@pytest.fixture(scope="module")
def lib():
    from pq_vector_amd import _ffi
    return _ffi.lib()


def brute(prows, pkeys, kind, a, b, q, d_all, gvalues, gvalid, k, m, allow=None):
    """The contract, group by group: every group's considered rows sorted by (distance key, position); the groups ranked by their
    first row; the first k, m rows each.  -> [(group value, [rows], [d2])]"""
    seq = pr.sequence(pkeys, kind, a, b, q)
    groups = {}
    for p, i in enumerate(seq):
        r = int(prows[i])
        if allow is not None and not allow[r]:
            continue
        if gvalid is not None and not gvalid[r]:
            continue
        bits = int(np.float32(d_all[r]).view(np.uint32))
        groups.setdefault(int(gvalues[r]), []).append((bits, p, r))
    ranked = sorted((sorted(v) for v in groups.values()), key=lambda v: v[0][:2])[:k]
    return [(int(gvalues[v[0][2]]), [r for _, _, r in v[:m]], [np.float32(d_all[r]) for _, _, r in v[:m]]) for v in ranked]


@pytest.mark.parametrize("name", ["1500x30", "2048x32-seq"])
def test_reference_is_the_contract(name):
    c = pgc.GroupCase(name, nq=5)
    allow = np.random.default_rng(9).random(c.n) < 0.5
    indexed = np.setdiff1d(np.arange(c.n), np.arange(5, c.n, 37))        # (as after a remove)
    for col in ("t3", "t64"):
        part = c.partition(col, indexed)
        for flt in c.filters(col):
            for gcol in pgc.GROUP_COLUMNS:
                gvalues, gvalid = c.groups[gcol]
                for (k, m), mask in (((10, 3), None), ((3, 1), allow), ((512, 2), allow)):
                    rows, dist, gkey, grows, nf, nc, considered, pass2 = c.grouped(part, flt, gcol, k, m, allow=mask)
                    n_cons = n_p2 = 0
                    for q in range(c.nq):
                        exp = brute(part[0], part[1], flt[1], flt[2], flt[3], q, c.d[q], gvalues, gvalid, k, m, mask)
                        assert nf[q] == len(exp) and nc[q] == len(pr.sequence(part[1], flt[1], flt[2], flt[3], q))
                        for g, (gv, er, ed) in enumerate(exp):
                            assert gkey[q, g] == gv and grows[q, g] == len(er) and rows[q, g, :len(er)].tolist() == er
                            assert (dist[q, g, :len(er)].view(np.uint32) == np.array(ed, np.float32).view(np.uint32)).all()
                            assert (rows[q, g, len(er):] == pgr.EMPTY).all() and np.isposinf(dist[q, g, len(er):]).all()
                        assert (rows[q, nf[q]:] == pgr.EMPTY).all() and (gkey[q, nf[q]:] == 0).all() and (grows[q, nf[q]:] == 0).all()
                        # the counts: what pass 1 and pass 2 evaluate
                        every = brute(part[0], part[1], flt[1], flt[2], flt[3], q, c.d[q], gvalues, gvalid, 10 ** 9, 10 ** 9, mask)
                        n_cons += sum(len(e[1]) for e in every)
                        n_p2 += sum(len(e[1]) for e in every if e[0] in {x[0] for x in exp})
                    assert (considered, pass2) == (n_cons, n_p2), (col, flt[0], gcol, k, m)


@pytest.mark.parametrize("name", list(pc.SHAPES))
def test_inputs_cover_what_the_gpu_tests_claim(name):
    c = pgc.GroupCase(name, nq=5)
    c.assert_distinct()
    g = c.groups
    assert g["doc32"][0].dtype == np.int32 and g["doc32"][1] is None and g["doc32"][0].min() < 0 < g["doc32"][0].max()
    assert set(np.unique(g["doc32"][0], return_counts=True)[1]) == {4}
    assert g["doc64"][0].dtype == np.int64 and np.abs(g["doc64"][0]).min() > 2 ** 31 and g["doc64"][0].min() < 0
    assert 0.1 < (g["doc64"][1] == 0).mean() < 0.3
    assert len(np.unique(g["few"][0])) == 5 and len(np.unique(g["single"][0])) == c.n and g["single"][1] is None
    # a document's chunks are scattered over the filter keys
    t3 = c.columns["t3"][0]
    assert np.mean([len(set(t3[g["doc32"][0] == v])) > 1 for v in np.unique(g["doc32"][0])[:200]]) > 0.5
    # n_found < k really occurs with `few`; some group has more than group_size considered rows, and some has fewer
    full = ("range", kf.RANGE, [kf.INT64_MIN] * c.nq, [kf.INT64_MAX] * c.nq)
    part = c.partition("t3")
    res = c.grouped(part, full, "few", 10, 3)
    assert (res[4] == 5).all() and (res[3][:, :5] == 3).all()
    res = c.grouped(part, full, "doc32", 10, 3)
    assert (res[4] == 10).all() and (res[3] == 3).all() and res[7] == 4 * 10 * c.nq, "groups of 4 rows cut to 3"
    res = c.grouped(part, c.filters("t3")[0], "doc32", 10, 3)
    assert ((res[3] > 0) & (res[3] < 3)).any(), "a group with fewer rows than group_size"


def test_tie_case_has_ties_inside_and_across_groups():
    data, queries, keys = pc.tie_case()
    groups = pgc.tie_groups()
    assert len(groups) == len(keys) and len(np.unique(groups)) == 7
    d = pr.distances("l2", pr.REF4, data, queries)
    near = np.argsort(d[0], kind="stable")[:50]
    assert len(np.unique(d[0][near])) < 10 and len(np.unique(groups[near])) > 1


def test_symbols_exported_bound_and_in_sys_rs(lib):
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
    # pqv_topk_partition's arities plus the group column, group_size, group_key and group_rows
    assert len(_ffi.SIGNATURES["pqv_topk_partition_grouped"][1]) == len(_ffi.SIGNATURES["pqv_topk_partition"][1]) + 4
    assert len(_ffi.SIGNATURES["pqv_topk_partition_grouped_device"][1]) == len(_ffi.SIGNATURES["pqv_topk_partition_device"][1]) + 4
    for f, needle in (("pq-vector_amd/csrc/Makefile", "kernels_partition_group.o"),
                      ("pq-vector_amd/csrc/kernels_all.hip", "kernels_partition_group.hip")):
        assert needle in open(os.path.join(ROOT, f)).read(), (f, needle)
    for m in ("topk_partition_grouped", "topk_partition_grouped_device", "topk_partition_distinct"):
        assert callable(getattr(pqv.Searcher, m))
    assert lib.pqv_abi_version() == 101


def test_c_abi_validates_in_the_stated_order_before_device_use(lib):
    from pq_vector_amd import _ffi
    inv = _ffi.PQV_ERR_INVALID
    fake = C.c_void_p(8)                 # never dereferenced: every check below comes before a handle is read
    zeros = (C.c_uint8 * 4096)()         # a handle whose owner is nobody: read by the ownership check only
    other = C.cast(zeros, C.c_void_p)
    nq = 2
    q = (C.c_float * (4 * nq))()
    rows, dist = (C.c_uint32 * (4 * nq))(), (C.c_float * (4 * nq))()

    def host(s, part, f, keys, k=2, m=2):
        return lib.pqv_topk_partition_grouped(s, part, f, keys, None, q, nq, 4, k, m, 0, 1, rows, dist, None, None, None, None)

    def device(s, part, f, keys, k=2, m=2):
        return lib.pqv_topk_partition_grouped_device(s, part, f, keys, None, None, nq, k, m, 0, 1, None, None, None, None, None, None, None)

    def flt(kind, a, b):
        return C.byref(_ffi.KeyFilter(kind, 0, C.cast(a, C.c_void_p) if a is not None else None,
                                      C.cast(b, C.c_void_p) if b is not None else None))

    def err(rc, text, code=inv):
        assert rc == code and text in lib.pqv_last_error(), (rc, lib.pqv_last_error())

    i64 = lambda *v: (C.c_int64 * len(v))(*v)       # noqa: E731
    u64 = lambda *v: (C.c_uint64 * len(v))(*v)      # noqa: E731
    good = flt(_ffi.PQV_KEY_EQ, i64(1, 2), None)
    for call, is_host in ((host, True), (device, False)):
        err(call(None, None, None, None), b"searcher must not be NULL")
        err(call(None, fake, good, fake), b"searcher must not be NULL")
        err(call(fake, None, None, None), b"key partition must not be NULL")
        err(call(fake, None, good, fake), b"key partition must not be NULL")
        err(call(fake, fake, None, None), b"row keys must not be NULL")
        err(call(fake, fake, good, None, k=0, m=0), b"row keys must not be NULL")
        err(call(fake, fake, None, fake), b"filter must not be NULL")
        err(call(fake, fake, flt(3, i64(1, 2), None), fake), b"unknown key filter kind 3")
        err(call(fake, fake, flt(_ffi.PQV_KEY_RANGE, i64(1, 2), None), fake), b"query keys must not be NULL")
        if is_host:
            err(call(fake, fake, flt(_ffi.PQV_KEY_IN, u64(0, 2, 1), i64(1, 2)), fake), b"query key sets must start at 0 and not decrease")
            # (the descriptor is checked ahead of k and group_size)
            err(call(fake, fake, flt(_ffi.PQV_KEY_IN, u64(0, 2, 4), i64(2, 1, 3, 4)), fake, k=0, m=0), b"query key sets must be strictly ascending")
        err(call(fake, fake, good, fake, k=0, m=0), b"k must be > 0")
        err(call(fake, fake, good, fake, k=2, m=0), b"group_size must be > 0")
        # the zero checks come before a handle is read, the ownership checks before the limits
        err(call(fake, other, good, fake), b"key partition belongs to another searcher")
        err(call(fake, other, good, fake, k=2 ** 31, m=2 ** 31), b"key partition belongs to another searcher")


def test_python_wrappers_check_their_arguments_before_device_use():
    import pq_vector_amd as pqv
    s = object.__new__(pqv.Searcher)       # no device here: the checks must come before the library is asked
    s._columns = {}
    q = np.zeros((2, 4), np.float32)
    fake = pqv.KeyPartition(8, s)          # (a handle that is never handed to the library)
    try:
        with pytest.raises(pqv.PqvError, match="part must be a KeyPartition"):
            s.topk_partition_grouped(q, 2, 2, pqv.RowKeys(None, s), pqv.RowKeys(None, s), query_keys=[1, 2])
        with pytest.raises(pqv.PqvError, match="query keys must not be NULL"):
            s.topk_partition_grouped(q, 2, 2, fake, pqv.RowKeys(None, s))
        with pytest.raises(pqv.PqvError, match="row keys must not be NULL"):
            s.topk_partition_grouped(q, 2, 2, fake, pqv.RowKeys(None, s), query_keys=[1, 2])
        with pytest.raises(pqv.PqvError, match="keys must be a RowKeys"):
            s.topk_partition_distinct(q, 2, fake, 5, query_keys=[1, 2])
        with pytest.raises(pqv.PqvError, match="no column named 'doc'"):
            s.topk_partition_distinct(q, 2, fake, "doc", query_keys=[1, 2])
        with pytest.raises(pqv.PqvError, match="keys must be a RowKeys"):
            s.topk_partition_grouped_device(8, 2, 2, 2, fake, "doc", 8, 8, query_keys=8)
    finally:
        fake._h = None
        s._h = None
