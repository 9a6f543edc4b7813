"""Candidate lists (pqv.h: pqv_topk_rows, pqv_score_rows), host side: the numpy restatement (tests/rows_ref.py) against
partition_ref (a list equal to a key's span) and mask_ref on the one-list index S1 of the contract's equivalence, the conditions on
the GPU tests' inputs (tests/rows_cases.py over tests/partition_cases.py), the ABI surface, the validation order -- all of it before
any device use -- and the Python wrapper's argument handling."""
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
import rows_cases as rc
import rows_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("pqv_topk_rows", "pqv_topk_rows_device", "pqv_score_rows", "pqv_score_rows_device")


@pytest.fixture(scope="module")
def lib():
    from pq_vector_amd import _ffi
    return _ffi.lib()


def test_restatement_is_the_contract():
    indexed = np.array([1, 1, 0, 1, 1, 1, 0, 1], bool)                # rows 2 and 6 are in no list (removed)
    d = np.array([5, 1, 0, 2, 1, 5, 0, 4], np.float32)
    cand = [7, 4, 2, 1, 4, 8, rr.EMPTY, 0, 5, 6]                      # unsorted, row 4 twice, 8 and 0xFFFFFFFF beyond the rows
    assert rr.considered(cand, indexed).tolist() == [True, True, False, True, True, False, False, True, True, False]
    r, dd, nf, nc, ncons = rr.topk(cand, indexed, d, 4)
    # (distance, position): row 4 at position 1, row 1 at 3, row 4 again at 4, then row 7
    assert (nf, nc, ncons) == (4, 10, 6) and r.tolist() == [4, 1, 4, 7] and dd.tolist() == [1, 1, 1, 4]
    r, dd, nf, nc, _ = rr.topk(cand, indexed, d, 8)
    assert nf == 6 and r.tolist() == [4, 1, 4, 7, 0, 5, rr.EMPTY, rr.EMPTY] and np.isposinf(dd[6:]).all()
    sc = rr.scores(cand, indexed, d)
    assert sc.tolist() == [4, 1, np.inf, 1, 1, np.inf, np.inf, 5, 5, np.inf]
    assert np.array_equal(rr.scores(cand, indexed, d, sqrt_out=True)[[0, 1]], np.sqrt(np.array([4, 1], np.float32)))
    # the mask: positions stay the unmasked ones, n_candidates is taken before it
    allow = np.ones(8, bool)
    allow[4] = False
    r, dd, nf, nc, ncons = rr.topk(cand, indexed, d, 3, allow=allow)
    assert (nf, nc, ncons) == (3, 10, 4) and r.tolist() == [1, 7, 0]
    assert np.isposinf(rr.scores(cand, indexed, d, allow=allow)[[1, 4]]).all()
    # the stable sort of the scores is the top-k
    r2, d2, nf2 = rr.topk_from_scores(cand, sc, 8)
    assert nf2 == 6 and r2.tolist() == rr.topk(cand, indexed, d, 8)[0].tolist()
    # lims need not start at 0
    lims, rows = rr.csr([[1, 2], [], [3]], base=4)
    assert lims.tolist() == [4, 6, 6, 7] and rows[4:].tolist() == [1, 2, 3] and len(rows) == 7
    # an empty list
    r, dd, nf, nc, _ = rr.topk([], indexed, d, 2)
    assert (nf, nc) == (0, 0) and r.tolist() == [rr.EMPTY] * 2


@pytest.mark.parametrize("name", ["4096x128", "2048x32-seq"])
def test_restatement_equals_the_partition_and_the_masked_restatements(name):
    """A list equal to one key's rows ascending is that key's span of the partition: partition_ref.topk with PQV_KEY_EQ.  An
    ascending unique list as the mask M_q on S1 (one list = all indexed rows ascending): mask_ref.masked_topk."""
    c = pc.Case(name)
    c.assert_distinct()
    indexed_rows = np.setdiff1d(np.arange(c.n), np.arange(5, c.n, 37))        # (as after a remove)
    indexed = np.zeros(c.n, bool)
    indexed[indexed_rows] = True
    shared = np.random.default_rng(9).random(c.n) < 0.5
    values, valid = c.columns["t3"]
    prows, pkeys = c.partition("t3", indexed_rows)
    keys = [-5, 0, 7, 3, 7][:c.nq]
    for allow in (None, shared):
        for k in (1, 10, 300):
            for q, key in enumerate(keys):
                span = prows[pr.sequence(pkeys, kf.EQ, keys, None, q)]
                assert (np.diff(span.astype(np.int64)) > 0).all()
                exp = pr.topk(prows, pkeys, kf.EQ, keys, None, q, c.d[q], k, "l2", False, allow)
                got = rr.topk(span, indexed, c.d[q], k, "l2", False, allow)
                assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(got, exp)), (k, q)
    lists = rc.unique_lists(c.n, rc.LENS_A, 11, ascending=True)
    for allow in (None, shared):
        for k in (1, 10, 300):
            for q, l in enumerate(lists[:c.nq]):
                m_q = np.zeros(c.n, bool)
                m_q[l] = True
                if allow is not None:
                    m_q &= allow
                er, ed, _, n_cons = mask_ref.masked_topk(indexed_rows.astype(np.uint32), m_q, c.data, c.queries[q], k, metric=c.metric)
                r, d, nf, nc, ncons = rr.topk(l, indexed, c.d[q], k, "l2", False, allow)
                assert nf == len(er) == min(k, n_cons) and ncons == n_cons and nc == len(l)
                assert (r[:nf] == er).all() and (d[:nf].view(np.uint32) == ed.view(np.uint32)).all()


def test_candidate_lists_cover_the_walk():
    assert set(rc.LENS_A) | set(rc.LENS_B) >= {0, 1, 63, 64, 65, 255, 256, 257}
    assert max(rc.LENS_A) >= 1000 and max(rc.LENS_B) >= 1000          # several turns of a block's 256 positions
    assert set(rc.KS) == {1, 10, 64, 65, 1024} and max(rc.KS) > max(rc.LENS_A)
    n = min(min(c["n"] for c in pc.SHAPES.values()), lrc.N)
    assert n > max(rc.LENS_B)
    for lens in (rc.LENS_A, rc.LENS_B):
        u = rc.unique_lists(n, lens, 3)
        assert [len(l) for l in u] == list(lens) and all(len(np.unique(l)) == len(l) and l.dtype == np.uint32 for l in u)
        assert any((np.diff(l.astype(np.int64)) < 0).any() for l in u), "unsorted lists"
        a = rc.unique_lists(n, lens, 3, ascending=True)
        assert all((np.diff(l.astype(np.int64)) > 0).all() for l in a)
        m = rc.messy_lists(n, lens, 4, bound=n - 1)
        assert [len(l) for l in m] == list(lens)
        big = m[-1]
        assert len(np.unique(big)) < len(big) and (big == rc.EMPTY).any() and (big == n).any() and (big == n + 1000).any()


@pytest.mark.parametrize("name", list(pc.SHAPES))
def test_inputs_have_no_equal_distances(name):
    pc.Case(name, 5).assert_distinct()


@pytest.mark.parametrize("name", pc.LONG_SHAPES)
def test_long_row_inputs_are_distinct(name, oracle):
    lrc.Case(name, oracle).assert_distinct()


def test_rows_symbols_exported_bound_and_in_sys_rs(lib):
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
    # pqv_topk_partition's arities with (lims, cand_rows) in place of (partition, filter); the score forms lose k and three outputs
    assert len(_ffi.SIGNATURES["pqv_topk_rows"][1]) == len(_ffi.SIGNATURES["pqv_topk_partition"][1])
    assert len(_ffi.SIGNATURES["pqv_topk_rows_device"][1]) == len(_ffi.SIGNATURES["pqv_topk_partition_device"][1])
    assert len(_ffi.SIGNATURES["pqv_score_rows"][1]) == len(_ffi.SIGNATURES["pqv_topk_rows"][1]) - 4
    assert len(_ffi.SIGNATURES["pqv_score_rows_device"][1]) == len(_ffi.SIGNATURES["pqv_topk_rows_device"][1]) - 4
    for f, needle in (("bindings/rust/src/lib.rs", "pub fn topk_rows"), ("bindings/rust/src/lib.rs", "pub fn score_rows"),
                      ("pq-vector_amd/host/pqv.hpp", "void topk_rows"), ("pq-vector_amd/host/pqv.hpp", "void score_rows"),
                      ("pq-vector_amd/csrc/Makefile", "kernels_rows.o"), ("pq-vector_amd/csrc/kernels_all.hip", "kernels_rows.hip")):
        assert needle in open(os.path.join(ROOT, f)).read(), (f, needle)
    for m in ("topk_rows", "score_rows", "topk_rows_device", "score_rows_device"):
        assert callable(getattr(pqv.Searcher, m))
    assert lib.pqv_abi_version() == 101


def test_rows_c_abi_validates_in_the_stated_order_before_device_use(lib):
    from pq_vector_amd import _ffi
    inv, uns = _ffi.PQV_ERR_INVALID, _ffi.PQV_ERR_UNSUPPORTED
    fake = C.c_void_p(8)                 # never dereferenced: every check it is passed to comes before a handle is read
    zeros = (C.c_uint8 * (1 << 20))()    # a handle whose owner is nobody / a searcher of dimension 0 that is no table: fields read, no device
    blank = C.cast(zeros, C.c_void_p)
    nq = 2
    q = (C.c_float * (4 * nq))()
    rows, dist = (C.c_uint32 * (2 * nq))(), (C.c_float * 16)()
    u64 = lambda *v: (C.c_uint64 * len(v))(*v)      # noqa: E731
    cand = (C.c_uint32 * 8)(*range(8))
    good = u64(3, 5, 8)                  # (need not start at 0)

    def topk(s, lims, cr, k=2, mask=None, metric=0, qlen=4, out=(rows, dist)):
        return lib.pqv_topk_rows(s, lims, cr, mask, q, nq, qlen, k, metric, 1, out[0], out[1], None, None)

    def topk_dev(s, lims, cr, k=2, mask=None, metric=0, qlen=4, out=(fake, fake)):
        return lib.pqv_topk_rows_device(s, C.cast(lims, C.c_void_p) if lims is not None else None, C.cast(cr, C.c_void_p) if cr is not None else None,
                                        mask, None, nq, k, metric, 1, out[0], out[1], None, None, None)

    def score(s, lims, cr, k=2, mask=None, metric=0, qlen=4, out=(None, dist)):
        return lib.pqv_score_rows(s, lims, cr, mask, q, nq, qlen, metric, 1, out[1])

    def score_dev(s, lims, cr, k=2, mask=None, metric=0, qlen=4, out=(None, fake)):
        return lib.pqv_score_rows_device(s, C.cast(lims, C.c_void_p) if lims is not None else None, C.cast(cr, C.c_void_p) if cr is not None else None,
                                         mask, None, nq, metric, 1, out[1], None)

    def err(rc, text, code=inv):
        assert rc == code and text in lib.pqv_last_error(), (rc, lib.pqv_last_error())

    for call, is_host, is_topk, who in ((topk, True, True, b"pqv_topk_rows"), (topk_dev, False, True, b"pqv_topk_rows"),
                                        (score, True, False, b"pqv_score_rows"), (score_dev, False, False, b"pqv_score_rows")):
        err(call(None, None, None), b"searcher must not be NULL")
        err(call(None, good, cand), b"searcher must not be NULL")
        err(call(fake, None, None), b"lims must not be NULL")
        err(call(fake, None, cand, k=0), b"lims must not be NULL")
        err(call(fake, good, None), b"cand_rows must not be NULL")
        err(call(fake, good, None, k=0), b"cand_rows must not be NULL")            # (ahead of k)
        if is_host:
            # every slice empty: cand_rows may be NULL, the next check speaks
            err(call(fake, u64(4, 4, 4), None, mask=blank), b"row mask belongs to another searcher")
            err(call(fake, u64(0, 2, 1), cand), b"lims must not decrease")
            err(call(fake, u64(5, 5, 4), cand), b"lims must not decrease")
            err(call(fake, u64(0, 1 << 32, 1 << 32), cand), b"a candidate list holds at most 2^32 - 1 rows")
            err(call(fake, u64(0, 2, 1), cand, mask=blank), b"lims must not decrease")      # (ahead of the mask)
        else:
            err(call(fake, u64(4, 4, 4), None), b"cand_rows must not be NULL")
        if is_topk:
            err(call(fake, good, cand, k=0), b"k must be > 0")
            err(call(fake, u64(0, 2, 1), cand, k=0), b"k must be > 0")              # (ahead of the slices)
        err(call(fake, good, cand, mask=blank), b"row mask belongs to another searcher")
        err(call(fake, good, cand, mask=blank, k=1025), b"row mask belongs to another searcher")
        # a blank searcher: no table, dimension 0 -- the remaining checks read its fields and no device
        err(call(blank, good, cand, metric=9), b"unknown metric")
        err(call(blank, good, cand, metric=9, k=1025), b"unknown metric")
        if is_host:
            err(call(blank, good, cand), b"Query dimension mismatch: expected 0, got 4")
            err(call(blank, good, cand, k=1025), b"Query dimension mismatch: expected 0, got 4")
        if is_topk:
            err(call(blank, good, cand, qlen=0, out=(None, dist)), b"row_idx/dist must not be NULL")
            err(call(blank, good, cand, qlen=0, out=(rows, None)), b"row_idx/dist must not be NULL")
            err(call(blank, good, cand, qlen=0, out=(None, None), k=1025), b"row_idx/dist must not be NULL")
            err(call(blank, good, cand, qlen=0, k=1025), who + b" takes k <= 1024", uns)
        else:
            err(call(blank, good, cand, qlen=0, out=(None, None)), b"dist must not be NULL")


def test_python_wrappers_check_their_arguments_before_device_use():
    import pq_vector_amd as pqv
    s = object.__new__(pqv.Searcher)       # no device here: the checks must come before the library is asked
    s._columns = {}
    s._h = None                            # (were a call to get through, the library would refuse the NULL searcher)
    q = np.zeros((2, 4), np.float32)
    try:
        for call in (lambda c, **kw: s.topk_rows(q, 2, c, **kw), lambda c, **kw: s.score_rows(q, c, **kw)):
            with pytest.raises(pqv.PqvError, match="candidates must not be None"):
                call(None)
            with pytest.raises(pqv.PqvError, match="candidates has 3 lists, the call has 2 queries"):
                call([[1], [2], [3]])
            with pytest.raises(pqv.PqvError, match="candidate row ids must be integers"):
                call([[1.5], [2]])
            with pytest.raises(pqv.PqvError, match=r"candidate row ids must be in \[0, 2\^32\)"):
                call([[-1], [2]])
            with pytest.raises(pqv.PqvError, match=r"candidate row ids must be in \[0, 2\^32\)"):
                call([[1], [2 ** 32]])
            with pytest.raises(pqv.PqvError, match="must be a pair"):
                call(([0, 1, 2], [1, 2], [3]))
            with pytest.raises(pqv.PqvError, match=r"lims must have nq \+ 1 = 3 entries"):
                call(([0, 1], [1, 2]))
            with pytest.raises(pqv.PqvError, match="lims must be non-negative integers"):
                call(([0.0, 1.0, 2.0], [1, 2]))
            with pytest.raises(pqv.PqvError, match="lims must be non-negative integers"):
                call(([-1, 1, 2], [1, 2]))
            with pytest.raises(pqv.PqvError, match="lims reach 5, the candidate rows hold 2 ids"):
                call(([0, 1, 5], [1, 2]))
            with pytest.raises(pqv.PqvError, match="sequence of per-query integer arrays"):
                call(5)
            with pytest.raises(pqv.PqvError, match="mask must be a RowMask"):
                call([[1], [2]], mask=np.ones(4, bool))
        from pq_vector_amd.api import _candidate_lists
        lims, rows = _candidate_lists([[3, 1, 1], [], np.array([0xFFFFFFFF], np.uint64)], 3)
        assert lims.dtype == np.uint64 and lims.tolist() == [0, 3, 3, 4] and rows.dtype == np.uint32 and rows.tolist() == [3, 1, 1, 0xFFFFFFFF]
        lims, rows = _candidate_lists((np.array([2, 4, 4]), [9, 9, 5, 6]), 2)
        assert lims.tolist() == [2, 4, 4] and rows.tolist() == [9, 9, 5, 6]
        lims, rows = _candidate_lists([], 0)
        assert lims.tolist() == [0] and rows.size == 0 and rows.dtype == np.uint32
    finally:
        s._h = None
