"""MMR top-k (pqv.h: pqv_mmr_select, pqv_topk_mmr), host side: the numpy restatement (tests/mmr_ref.py) on a hand-written case, the
conditions on the GPU tests' candidate sets (tests/mmr_cases.py), the ABI surface, the validation order -- all of it before any
device use -- and the Python wrappers' argument handling."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mmr_cases as mc
import mmr_ref as mr
import partition_cases as pc
from range_oracle import REF4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("pqv_mmr_select", "pqv_mmr_select_device", "pqv_topk_mmr", "pqv_topk_mmr_device")


@pytest.fixture(scope="module")
def lib():
    from pq_vector_amd import _ffi
    return _ffi.lib()


def _hand(k, lam, n_found_in=mc.HAND_N_FOUND_IN):
    pd = mr.Pairwise("l2", REF4, mc.HAND_ROWS, False)
    r, d, s, nf = mr.select(mc.HAND_CAND, mc.HAND_REL, k, lam, mc.HAND_INDEXED, pd, n_found_in)
    return r.tolist(), d.tolist(), s.tolist(), nf


def test_restatement_on_the_hand_written_case():
    """Rows r0 (1,0), r1 (1,1), r2 (-2,0), r3 (0,3), r4 (2,2: in no list), r5 (3,0); the query is the origin, distances are d2.
    Candidates by position: 0:r0 1:r1 2:r0 3:r2 4:r4 5:r3 6:r5 with rel 1 2 1 4 8 9 9 and n_found_in 6, so the considered
    positions are 0, 1, 2, 3 and 5 (4 is unindexed, 6 is beyond n_found_in).
    pd: (r0,r1) 1, (r0,r0) 0, (r0,r2) 9, (r0,r3) 10, (r2,r1) 10, (r2,r3) 13, (r3,r1) 5.

    lambda 1: score = rel; by (rel, position): 0 (1), 2 (1), 1 (2), 3 (4), 5 (9).
    lambda 0: score = 0 - red.  Step 0: all +0, position 0 wins.  red = [1, 0, 9, 10] at positions 1, 2, 3, 5, scores -1, +0, -9, -10:
      position 5 (r3).  red = [min(1,5), min(0,10), min(9,13)] = [1, 0, 9]: position 3 (r2, -9).  red = [min(1,10), min(0,9)]: position
      1 (-1), then position 2, whose red is pd(r0, r0) = 0: score +0.
    lambda 0.5: step 0 scores .5 1 .5 2 4.5: position 0.  Then .5*rel - .5*red = 1 - .5, .5 - 0, 2 - 4.5, 4.5 - 5 = .5, .5, -2.5, -.5:
      position 3 (r2).  red at 1, 2, 5 = 1, 0, min(10, 13) = 10: scores .5, .5, -.5: position 5.  Then .5 and .5 tie: position 1, then 2."""
    E, inf = mr.EMPTY, np.inf
    assert _hand(4, 1.0) == ([0, 0, 1, 2], [1, 1, 2, 4], [1, 1, 2, 4], 4)
    assert _hand(8, 1.0) == ([0, 0, 1, 2, 3, E, E, E], [1, 1, 2, 4, 9, inf, inf, inf], [1, 1, 2, 4, 9, inf, inf, inf], 5)
    r, d, s, nf = _hand(5, 0.0)
    assert (r, d, nf) == ([0, 3, 2, 1, 0], [1, 9, 4, 2, 1], 5) and s == [0, -10, -9, -1, 0]
    assert np.array(s, np.float32).view(np.uint32)[[0, 4]].tolist() == [0, 0], "0 - 0 is +0"
    assert _hand(5, 0.5) == ([0, 2, 3, 1, 0], [1, 4, 9, 2, 1], [0.5, -2.5, -0.5, 0.5, 0.5], 5)
    assert _hand(2, 0.5) == ([0, 2], [1, 4], [0.5, -2.5], 2)
    # without n_found_in position 6 (r5: pd (r0,r5) 4, rel 9) is considered too; an n_found_in beyond n is n
    assert _hand(8, 1.0, None)[0] == [0, 0, 1, 2, 3, 5, E, E] and _hand(8, 1.0, 100) == _hand(8, 1.0, None)
    assert _hand(8, 0.0, 0) == ([E] * 8, [inf] * 8, [inf] * 8, 0)
    # the first pick is the smallest (ord(lambda * rel), position) whatever lambda is
    for lam in (0.0, 0.3, 0.5, 1.0):
        assert _hand(1, lam)[0] == [0]


def test_lambda_one_is_the_input_order():
    c = pc.Case("1500x30", 3)
    indexed = np.ones(c.n, bool)
    pd = mr.Pairwise("l2", c.metric, c.data, True)
    for q in range(c.nq):
        cand = mc.nearest(c.d[q], "l2", np.arange(c.n), 65)
        rel = mc.rel_of(cand, c.d[q], "l2", True)
        assert (np.diff(rel) > 0).all()
        r, d, s, nf = mr.select(cand, rel, 10, 1.0, indexed, pd)
        assert nf == 10 and (r == cand[:10]).all() and (d.view(np.uint32) == rel[:10].view(np.uint32)).all() and (s == d).all()
        # a smaller lambda moves away from it, and never changes the first pick
        r3 = mr.select(cand, rel, 10, 0.3, indexed, pd)[0]
        assert r3[0] == cand[0] and (r3 != cand[:10]).any() and len(set(r3.tolist())) == 10


def test_nan_pd_leaves_the_running_minimum():
    indexed = np.ones(3, bool)
    table = {0: np.array([np.nan, 4.0], np.float32), 1: np.array([np.nan], np.float32)}
    pd = lambda row, against: table[row][:len(against)]      # noqa: E731
    r, d, s, nf = mr.select([0, 1, 2], [1, 2, 3], 3, 0.5, indexed, pd)
    # after the first pick red = [inf (NaN never compares smaller), 4]: scores 1 - inf = -inf, 1.5 - 2 = -.5
    assert r.tolist() == [0, 1, 2] and s.tolist() == [0.5, -np.inf, -0.5] and nf == 3


def test_candidate_sets_cover_the_kernel_paths():
    assert set(mc.NS) == {1, 63, 64, 65, 257, 1024} and set(mc.LAMBDAS) == {0.0, 0.3, 0.5, 1.0}
    n_rows = 1500
    d = np.random.default_rng(1).random(n_rows, dtype=np.float32)
    c = mc.nearest(d, "l2", np.arange(n_rows), 1024)
    assert len(c) == 1024 and (np.diff(d[c]) >= 0).all() and len(np.unique(c)) == 1024
    assert (np.diff(mc.shuffled(c, 3).astype(np.int64)) < 0).any() and sorted(mc.shuffled(c, 3)) == sorted(c)
    dup = mc.with_duplicates(c, 4)
    assert len(dup) == 1024 and len(np.unique(dup)) < 1024 and (dup[4::5] == dup[0]).all()
    m = mc.messy(c, n_rows, 5, removed=[7])
    assert (m == mc.EMPTY).any() and (m == n_rows).any() and (m == n_rows + 1000).any() and (m == 7).any()
    rel = mc.rel_of(m, d, "l2", True)
    assert (rel[m >= n_rows] == 0).all() and (rel[m < n_rows] == np.sqrt(d[m[m < n_rows]])).all()
    assert mc.HAND_INDEXED.sum() == 5 and len(mc.HAND_CAND) == len(mc.HAND_REL) == 7 and mc.HAND_N_FOUND_IN < 7
    assert (mc.HAND_REL == (mc.HAND_ROWS[mc.HAND_CAND] ** 2).sum(1)).all()


def _arity(text, name, opener):
    """the parameter count of `name` in a C header or sys.rs: commas at depth 0 of its parenthesised list, comments dropped"""
    at = re.search(opener % name, text)
    assert at, name
    i = text.index("(", at.start())
    depth, j = 0, i
    while True:
        depth += {"(": 1, ")": -1}.get(text[j], 0)
        if depth == 0:
            break
        j += 1
    params = re.sub(r"/\*.*?\*/", "", text[i + 1:j], flags=re.S)
    return params.count(",") + 1


def test_mmr_symbols_exported_bound_and_in_sys_rs(lib):
    from pq_vector_amd import _ffi
    import pq_vector_amd as pqv
    hdr = open(os.path.join(ROOT, "include", "pqv.h")).read()
    sys_rs = open(os.path.join(ROOT, "bindings", "rust", "src", "sys.rs")).read()
    raw = C.CDLL(_ffi.LIB_PATH)
    for name, arity in zip(NEW_SYMBOLS, (14, 15, 17, 17)):
        assert hasattr(raw, name), name
        assert name in _ffi.SIGNATURES
        assert getattr(lib, name).argtypes == _ffi.SIGNATURES[name][1]
        assert len(_ffi.SIGNATURES[name][1]) == arity
        assert _arity(hdr, name, r"\bint %s\s*\(") == arity, name
        assert _arity(sys_rs, name, r"pub fn %s\(") == arity, name
    for f, needle in (("bindings/rust/src/lib.rs", "pub fn topk_mmr"), ("bindings/rust/src/lib.rs", "pub fn mmr_select"),
                      ("pq-vector_amd/host/pqv.hpp", "void topk_mmr"), ("pq-vector_amd/host/pqv.hpp", "void mmr_select"),
                      ("pq-vector_amd/csrc/Makefile", "kernels_mmr.o"), ("pq-vector_amd/csrc/Makefile", "kernels_mmr.hip"),
                      ("pq-vector_amd/csrc/kernels_all.hip", "kernels_mmr.hip"), ("pq-vector_amd/csrc/kernels.h", "launch_mmr_select")):
        assert needle in open(os.path.join(ROOT, f)).read(), (f, needle)
    for m in ("topk_mmr", "mmr_select", "topk_mmr_device", "mmr_select_device"):
        assert callable(getattr(pqv.Searcher, m))
    assert callable(pqv.TopkBuilder.mmr)
    assert lib.pqv_abi_version() == 101


def test_mmr_c_abi_validates_in_the_stated_order_before_device_use(lib):
    from pq_vector_amd import _ffi
    inv, uns = _ffi.PQV_ERR_INVALID, _ffi.PQV_ERR_UNSUPPORTED
    fake = C.c_void_p(8)                 # never dereferenced: every check it is passed to comes before a handle is read
    zeros = (C.c_uint8 * (1 << 20))()    # a handle whose owner is nobody / a searcher of dimension 0 that is no table: fields read, no device
    blank = C.cast(zeros, C.c_void_p)
    nq, n = 2, 4
    q = (C.c_float * (4 * nq))()
    cand, rel = (C.c_uint32 * (n * nq))(), (C.c_float * (n * nq))()
    rows, dist = (C.c_uint32 * (2048 * nq))(), (C.c_float * (2048 * nq))()
    nan = float("nan")

    def select(s, k=2, n=n, lam=0.5, metric=0, cr=(cand, rel), out=(rows, dist), **_):
        return lib.pqv_mmr_select(s, cr[0], cr[1], None, nq, n, k, lam, metric, 1, out[0], out[1], None, None)

    def select_dev(s, k=2, n=n, lam=0.5, metric=0, cr=(fake, fake), out=(fake, fake), **_):
        return lib.pqv_mmr_select_device(s, cr[0], cr[1], None, nq, n, k, lam, metric, 1, out[0], out[1], None, None, None)

    def fused(s, k=2, n=n, lam=0.5, metric=0, mask=None, nprobe=1, qlen=4, out=(rows, dist), queries=q, **_):
        return lib.pqv_topk_mmr(s, mask, queries, nq, qlen, k, n, lam, nprobe, 0, metric, 1, out[0], out[1], None, None, None)

    def fused_dev(s, k=2, n=n, lam=0.5, metric=0, mask=None, nprobe=1, out=(fake, fake), queries=fake, **_):
        return lib.pqv_topk_mmr_device(s, mask, queries, nq, k, n, lam, nprobe, 0, metric, 1, out[0], out[1], None, None, None, None)

    def err(rc, text, code=inv):
        assert rc == code and text in lib.pqv_last_error(), (rc, lib.pqv_last_error())

    for call, is_fused, is_host, who in ((select, False, True, b"pqv_mmr_select"), (select_dev, False, False, b"pqv_mmr_select"),
                                         (fused, True, True, b"pqv_topk_mmr"), (fused_dev, True, False, b"pqv_topk_mmr")):
        limit = who + (b" takes fetch_k <= 1024" if is_fused else b" takes n <= 1024")
        err(call(None), b"searcher must not be NULL")
        err(call(None, k=0, lam=2.0), b"searcher must not be NULL")
        err(call(fake, k=0), b"k must be > 0")
        err(call(fake, k=0, lam=nan, n=2000), b"k must be > 0")
        if is_fused:
            err(call(fake, k=5, n=4), b"fetch_k must be >= k")
            err(call(fake, k=5, n=4, lam=-1.0), b"fetch_k must be >= k")              # (ahead of lambda)
            err(call(fake, k=2000, n=1999), b"fetch_k must be >= k")                  # (ahead of the limit)
        else:
            err(call(fake, k=5, n=4, lam=-1.0), b"lambda must be in [0, 1]")          # (n < k is fine for the selection)
        for bad in (nan, -0.25, 1.5, float("inf")):
            err(call(fake, lam=bad), b"lambda must be in [0, 1]")
        err(call(fake, lam=nan, n=1025), b"lambda must be in [0, 1]")                 # (ahead of the limit)
        err(call(fake, n=1025), limit, uns)
        err(call(fake, n=1025, k=1025), limit, uns)
        if is_fused:
            err(call(fake, n=1025, mask=blank), limit, uns)                            # (ahead of the mask)
            err(call(fake, mask=blank), b"row mask belongs to another searcher")
            err(call(fake, mask=blank, nprobe=0), b"row mask belongs to another searcher")
            # a blank searcher: no table, dimension 0, no clusters -- the remaining checks read its fields and no device
            err(call(blank, nprobe=0), b"nprobe must be > 0")
            err(call(blank, nprobe=0, metric=9), b"nprobe must be > 0")
        err(call(blank, metric=9), b"unknown metric")
        for lam in (0.0, 1.0):                                                        # (both ends are inside)
            err(call(blank, metric=9, lam=lam), b"unknown metric")
        if is_fused and is_host:
            err(call(blank), b"Query dimension mismatch: expected 0, got 4")
            err(call(blank, out=(None, None)), b"Query dimension mismatch: expected 0, got 4")
            err(call(blank, qlen=0, out=(None, dist)), b"queries/row_idx/dist must not be NULL")
            err(call(blank, qlen=0, queries=None), b"queries/row_idx/dist must not be NULL")
        elif is_fused:
            err(call(blank, out=(None, fake)), b"device pointers must not be NULL")
            err(call(blank, queries=None), b"device pointers must not be NULL")
        else:
            err(call(blank, cr=(None, rel) if is_host else (None, fake)), b"cand_rows/cand_dist must not be NULL")
            err(call(blank, cr=(cand, None) if is_host else (fake, None)), b"cand_rows/cand_dist must not be NULL")
            err(call(blank, out=(None, dist) if is_host else (None, fake)), b"row_idx/dist must not be NULL")
            err(call(blank, out=(rows, None) if is_host else (fake, None)), b"row_idx/dist must not be NULL")


def test_python_wrappers_check_their_arguments_before_device_use():
    import pq_vector_amd as pqv
    s = object.__new__(pqv.Searcher)       # no device here: the checks must come before the library is asked
    s._columns = {}
    s._h = None                            # (a call that gets through is refused by the library: the NULL searcher)
    rows = np.arange(8, dtype=np.uint32).reshape(2, 4)
    dist = np.ones((2, 4), np.float32)
    with pytest.raises(pqv.PqvError, match="rows and dist of one"):
        s.mmr_select(rows, dist[:, :3], 2)
    with pytest.raises(pqv.PqvError, match="rows and dist of one"):
        s.mmr_select(rows.reshape(2, 2, 2), dist.reshape(2, 2, 2), 2)
    with pytest.raises(pqv.PqvError, match="n_found of length 2, got 3"):
        s.mmr_select(rows, dist, 2, n_found=[1, 2, 3])
    # well-formed arguments reach the library, which speaks first of the searcher, then of the arguments in the contract's order
    for call in (lambda: s.mmr_select(rows, dist, 2, n_found=[4, 2]), lambda: s.mmr_select(rows[0], dist[0], 2, lambda_=1),
                 lambda: s.topk_mmr(np.zeros((2, 4), np.float32), 2, 10, 1), lambda: s.topk_mmr(np.zeros(4, np.float32), 2, 10, 1, lambda_=0.0),
                 lambda: s.topk_mmr_device(0, 2, 2, 10, 1, 0, 0), lambda: s.mmr_select_device(0, 0, 2, 4, 2, 0, 0)):
        with pytest.raises(pqv.PqvError, match="searcher must not be NULL"):
            call()
    with pytest.raises(pqv.PqvError, match="mask must be a RowMask"):
        s.topk_mmr(np.zeros((2, 4), np.float32), 2, 10, 1, mask=np.ones(4, bool))


def test_topk_builder_mmr_composes_and_refuses():
    import pq_vector_amd as pqv
    src = object()                         # a Searcher source that is never asked: every refusal comes first
    q = np.zeros(4, np.float32)
    b = pqv.TopkBuilder(src, q).k(2).nprobe(1)
    assert b.mmr(10) is b and b._mmr == (10, 0.5) and b.mmr(7, lambda_=1)._mmr == (7, 1.0)
    with pytest.raises(pqv.PqvError, match="fetch_k must be > 0"):
        b.mmr(0)
    for bad in (-0.1, 1.1, float("nan")):
        with pytest.raises(pqv.PqvError, match=r"lambda must be in \[0, 1\]"):
            b.mmr(10, lambda_=bad)
    with pytest.raises(pqv.PqvError, match=r"mmr\(\) does not combine with distinct_on\(\)") as e:
        pqv.TopkBuilder(src, q).k(2).nprobe(1).distinct_on("doc").mmr(10).search()
    from pq_vector_amd import _ffi
    assert e.value.code == _ffi.PQV_ERR_UNSUPPORTED and "mmr_select" in str(e.value)
    with pytest.raises(pqv.PqvError, match=r"mmr\(\) does not combine with distinct_on\(\)"):
        pqv.TopkBuilder(src, q).k(2).nprobe(1).mmr(10).distinct_on("doc").group_size(2).search()
    with pytest.raises(pqv.PqvError, match=r"mmr\(\) does not combine with max_nprobe\(\)"):
        pqv.TopkBuilder(src, q).k(2).nprobe(1).mmr(10).max_nprobe(4).search()
    with pytest.raises(pqv.PqvError, match="pqv_topk_mmr does not take table searchers"):
        pqv.TableTopkBuilder(["a.parquet", "b.parquet"], q).k(2).nprobe(1).mmr(10).search()
