"""Row-masked search, host side: the numpy restatement (tests/mask_ref.py) pinned to the C oracle through the filtered-lists
setup, the ABI surface, argument validation that needs no device, and the Parquet predicate -> row mask conversion."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mask_ref
from range_oracle import REF4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("pqv_row_mask_create", "pqv_row_mask_from_device", "pqv_row_mask_rows", "pqv_row_mask_count", "pqv_row_mask_free",
               "pqv_topk_masked", "pqv_topk_masked_device", "pqv_range_search_masked")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def lib():
    from pq_vector_amd import _ffi
    return _ffi.lib()


def _masks(rng, n):
    """several selectivities, all-false and all-true"""
    out = {f"1/{d}": rng.random(n) < 1.0 / d for d in (64, 8, 2)}
    out["63/64"] = rng.random(n) < 63.0 / 64
    out["none"] = np.zeros(n, dtype=bool)
    out["all"] = np.ones(n, dtype=bool)
    return out


@pytest.mark.parametrize("dim", [3, 30, 128])
def test_restatement_equals_the_oracle_on_the_filtered_lists_index(oracle, dim):
    """Random f32 data (distinct distances, asserted): masked top-k over candidate_rows, capped then masked, ordered by
    (d2, original position) == oracle.topk on the index whose lists are intersected with the allowed rows -- rows and bits."""
    rng = np.random.default_rng(100 + dim)
    n, kc = 700, 7
    data = rng.random((n, dim), dtype=np.float32)
    oidx = oracle.build_index(data, n_clusters=kc, max_iters=5, workers=1)
    queries = rng.random((6, dim), dtype=np.float32)
    for name, allowed in _masks(rng, n).items():
        filt = oracle.index_from_parts(dim, oidx.centroids, mask_ref.filtered_lists(oidx.lists(), allowed))
        for q in queries:
            for k, nprobe in ((1, 1), (10, 3), (100, kc), (300, 2)):
                cand = oidx.candidate_rows(q, nprobe)
                rows_c, _ = mask_ref.considered(cand, allowed)
                _, d2_all, _, _ = mask_ref.masked_topk(cand, allowed, data, q, max(1, len(rows_c)))
                assert len(np.unique(_bits(d2_all))) == len(d2_all), "expected distances must be distinct"
                rows, d2, n_cand, n_cons = mask_ref.masked_topk(cand, allowed, data, q, k)
                orows, odist, onc = filt.topk(data, q, k, nprobe)
                assert n_cand == len(cand) and n_cons == onc == len(rows_c), name
                assert (rows == orows).all() and len(rows) == len(orows) == min(k, n_cons), name
                assert (_bits(np.sqrt(d2)) == _bits(odist)).all(), name
                if name == "none":
                    assert len(rows) == 0
                if name == "all":
                    arows, adist, _ = oidx.topk(data, q, k, nprobe)
                    assert (rows == arows).all() and (_bits(np.sqrt(d2)) == _bits(adist)).all()


def test_heap_over_the_filtered_sequence_equals_the_filtered_lists_index_under_ties(oracle):
    """Tie-heavy integer data: the reference's heap over the filtered candidate sequence (pqo_topk_df: arrival order) keeps the
    rows oracle.topk keeps on the filtered-lists index -- a monotone map of positions preserves heap arrival order."""
    rng = np.random.default_rng(5)
    cases = 0
    for dim in (3, 8):
        for n, kc in ((300, 5), (120, 9)):
            data = rng.integers(0, 3, (n, dim)).astype(np.float32)
            oidx = oracle.build_index(data, n_clusters=kc, max_iters=5, workers=1)
            lists = oidx.lists()
            for allowed in _masks(rng, n).values():
                flists = mask_ref.filtered_lists(lists, allowed)
                filt = oracle.index_from_parts(dim, oidx.centroids, flists)
                for q in rng.integers(0, 3, (5, dim)).astype(np.float32):
                    for k, nprobe in ((1, 1), (5, 2), (40, kc)):
                        rows_c, _ = mask_ref.considered(oidx.candidate_rows(q, nprobe), allowed)
                        drows, dd2 = oracle.topk_df(data, rows_c, q, k)
                        orows, odist, _ = filt.topk(data, q, k, nprobe)
                        assert (drows == orows).all() and len(drows) == len(orows)
                        assert (_bits(np.sqrt(dd2)) == _bits(odist)).all()       # (integer data: both chains are exact)
                        cases += 1
    assert cases >= 360


def test_restatement_caps_before_it_masks():
    cand = np.array([5, 1, 4, 2, 0, 3], np.uint32)
    allowed = np.array([1, 0, 1, 1, 0, 1], bool)
    rows, pos = mask_ref.considered(cand, allowed, max_candidates=4)
    assert rows.tolist() == [5, 2] and pos.tolist() == [0, 3]
    data = np.arange(6, dtype=np.float32).reshape(6, 1)
    r, d2, nc, ncons = mask_ref.masked_topk(cand, allowed, data, np.zeros(1, np.float32), 3, max_candidates=4)
    assert r.tolist() == [2, 5] and d2.tolist() == [4.0, 25.0] and nc == 6 and ncons == 2
    r, out, nw, nc = mask_ref.masked_range(cand, allowed, data, np.zeros(1, np.float32), 2.5, max_candidates=4)
    assert r.tolist() == [2] and out.tolist() == [2.0] and nw == 1 and nc == 6


def test_mask_symbols_exported_bound_and_in_sys_rs(lib):
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
    assert len(_ffi.SIGNATURES["pqv_topk_masked"][1]) == len(_ffi.SIGNATURES["pqv_topk"][1]) + 1
    assert len(_ffi.SIGNATURES["pqv_topk_masked_device"][1]) == len(_ffi.SIGNATURES["pqv_topk_device_flags"][1]) + 1
    assert len(_ffi.SIGNATURES["pqv_range_search_masked"][1]) == len(_ffi.SIGNATURES["pqv_range_search"][1]) + 1
    assert "typedef struct pqv_row_mask pqv_row_mask;" in hdr and "pub struct PqvRowMask" in sys_rs
    for f, needle in (("bindings/rust/src/lib.rs", "pub struct RowMask"), ("bindings/rust/src/lib.rs", "impl Drop for RowMask"),
                      ("pq-vector_amd/host/pqv.hpp", "class RowMask")):
        assert needle in open(os.path.join(ROOT, f)).read(), (f, needle)
    assert lib.pqv_abi_version() == 101


def test_mask_c_abi_validates_before_device_use(lib):
    from pq_vector_amd import _ffi
    inv = _ffi.PQV_ERR_INVALID
    h = C.c_void_p()
    allowed = (C.c_uint8 * 4)()
    assert lib.pqv_row_mask_create(None, allowed, 4, C.byref(h)) == inv and b"searcher must not be NULL" in lib.pqv_last_error()
    assert lib.pqv_row_mask_from_device(None, None, 4, None, C.byref(h)) == inv and b"searcher must not be NULL" in lib.pqv_last_error()
    fake = C.c_void_p(8)         # never dereferenced: the NULL checks come first
    assert lib.pqv_row_mask_create(None, allowed, 4, None) == inv and b"out must not be NULL" in lib.pqv_last_error()
    assert lib.pqv_row_mask_from_device(None, None, 4, None, None) == inv and b"out must not be NULL" in lib.pqv_last_error()
    q = (C.c_float * 4)()
    rows, dist = (C.c_uint32 * 2)(), (C.c_float * 2)()
    rc = lib.pqv_topk_masked(None, fake, q, 1, 4, 2, 1, 0, 0, 1, rows, dist, None, None)
    assert rc == inv and b"searcher must not be NULL" in lib.pqv_last_error()
    rc = lib.pqv_topk_masked_device(None, fake, None, 1, 2, 1, 0, 0, 1, None, None, None, None, None, None)
    assert rc == inv and b"searcher must not be NULL" in lib.pqv_last_error()
    lims, rr, dd = _ffi.u64p(), _ffi.u32p(), _ffi.f32p()
    rc = lib.pqv_range_search_masked(None, fake, q, 1, 4, 1.0, 1, 0, 0, 0, 1, C.byref(lims), C.byref(rr), C.byref(dd), None, None)
    assert rc == inv and b"searcher must not be NULL" in lib.pqv_last_error()
    # a NULL mask: refused before the searcher is touched (the handle here is never dereferenced)
    rc = lib.pqv_topk_masked(fake, None, q, 1, 4, 2, 1, 0, 0, 1, rows, dist, None, None)
    assert rc == inv and b"row mask must not be NULL" in lib.pqv_last_error()
    rc = lib.pqv_topk_masked_device(fake, None, None, 1, 2, 1, 0, 0, 1, None, None, None, None, None, None)
    assert rc == inv and b"row mask must not be NULL" in lib.pqv_last_error()
    rc = lib.pqv_range_search_masked(fake, None, q, 1, 4, 1.0, 1, 0, 0, 0, 1, C.byref(lims), C.byref(rr), C.byref(dd), None, None)
    assert rc == inv and b"row mask must not be NULL" in lib.pqv_last_error()
    assert lib.pqv_row_mask_rows(None) == 0 and lib.pqv_row_mask_count(None) == 0
    lib.pqv_row_mask_free(None)


class _FakeCorpus:
    rows = 6


def _fake_searcher(pqv):
    s = object.__new__(pqv.Searcher)       # no device here: the checks must come before the library is asked
    s._h, s.dim, s.n_clusters, s._corpus = None, 4, 2, _FakeCorpus()
    return s


def test_python_mask_arguments_are_checked_before_device_use():
    import pq_vector_amd as pqv
    assert pqv.RowMask in (getattr(pqv, n) for n in pqv.__all__)
    s = _fake_searcher(pqv)
    with pytest.raises(pqv.PqvError, match="row mask has 5 rows, the corpus has 6") as e:
        s.row_mask(np.zeros(5, bool))
    assert e.value.code == -1
    with pytest.raises(pqv.PqvError, match="bool or uint8"):
        s.row_mask(np.zeros(6, np.int64))
    with pytest.raises(pqv.PqvError, match="must not be None"):
        s.row_mask(None)
    with pytest.raises(pqv.PqvError, match="row id out of range"):
        s.row_mask_from_rows([1, 6])
    with pytest.raises(pqv.PqvError, match="mask must be a RowMask"):
        s.topk(np.zeros((1, 4), np.float32), 2, 1, mask=np.ones(6, bool))
    with pytest.raises(pqv.PqvError, match="mask must be a RowMask"):
        s.range_search(np.zeros((1, 4), np.float32), 1.0, 1, mask=np.ones(6, bool))
    closed = pqv.RowMask(None, s)
    with pytest.raises(pqv.PqvError, match="row mask must not be NULL"):
        s.topk(np.zeros((1, 4), np.float32), 2, 1, mask=closed)
    assert closed.rows == 0 and closed.count == 0
    closed.close()
    s._h = None


@pytest.fixture
def six_row_file(tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    path = str(tmp_path / "six.parquet")
    vec = pa.array([[float(i), 0.0] for i in range(6)], type=pa.list_(pa.float32()))
    pq.write_table(pa.table({"id": pa.array([0, 1, 2, 3, None, 5], type=pa.int64()), "vec": vec}), path, row_group_size=4)
    assert pq.ParquetFile(path).metadata.num_row_groups == 2
    return path


def test_row_mask_from_expression_keeps_file_row_order_and_nulls_are_false(six_row_file):
    import pyarrow.compute as pc
    import pq_vector_amd as pqv
    from pq_vector_amd import parquet_io
    m = parquet_io.row_mask_from_expression(six_row_file, pc.field("id") >= 2)
    assert m.dtype == np.bool_ and m.tolist() == [False, False, True, True, False, True]
    assert parquet_io.row_mask_from_expression(six_row_file, pc.field("id") < 0).tolist() == [False] * 6
    with pytest.raises(pqv.PqvError, match="must be boolean"):
        parquet_io.row_mask_from_expression(six_row_file, pc.field("id") + 1)
    with pytest.raises(pqv.PqvError, match="cannot evaluate the predicate"):
        parquet_io.row_mask_from_expression(six_row_file, pc.field("nope") >= 2)
    with pytest.raises(pqv.PqvError, match="needs a pyarrow.compute.Expression"):
        parquet_io.row_mask_from_expression(six_row_file, "id >= 2")


def test_where_validation_on_all_four_builders(six_row_file):
    import pyarrow.compute as pc
    import pq_vector_amd as pqv
    q = np.zeros(2, np.float32)
    expr = pc.field("id") >= 2
    ok = np.array([0, 0, 1, 1, 0, 1], bool)
    s = _fake_searcher(pqv)
    other = _fake_searcher(pqv)
    for make in (lambda src: pqv.TopkBuilder(src, q), lambda src: pqv.RangeBuilder(src, q)):
        b = make(six_row_file)
        assert b.where(ok) is b and b.where(expr) is b
        for bad, text in ((None, "got None"), (np.zeros(6, np.uint8), "needs a bool array"), (np.zeros(5, bool), "row mask has 5 rows, the corpus has 6"),
                          ("id >= 2", "needs a bool array"), (pqv.RowMask(None, s), "needs a Searcher source")):
            before = b._where
            with pytest.raises(pqv.PqvError, match=text) as e:
                b.where(bad)
            assert e.value.code == -1 and b._where is before          # a refusal changes nothing
        b = make(s)
        mine = pqv.RowMask(None, s)
        assert b.where(mine) is b and b._where is mine and b.where(ok) is b
        with pytest.raises(pqv.PqvError, match="row mask belongs to another searcher"):
            b.where(pqv.RowMask(None, other))
        with pytest.raises(pqv.PqvError, match="needs a Parquet path source"):
            b.where(expr)
        with pytest.raises(pqv.PqvError, match="row mask has 7 rows, the corpus has 6"):
            b.where(np.zeros(7, bool))
        assert make(six_row_file)._where is None                      # without where(): today's path
    for make in (lambda: pqv.TableTopkBuilder([six_row_file, six_row_file], q), lambda: pqv.TableRangeBuilder([six_row_file, six_row_file], q)):
        b = make()
        assert b._where is None
        assert b.where(expr) is b and len(b._where) == 2
        assert b.where([ok, expr]) is b
        for bad, text in ((None, "got None"), ([ok], "1 entries for 2 files"), (ok, "one bool array / expression per file"),
                          ([ok, np.zeros(5, bool)], "row mask has 5 rows"), ([ok, np.zeros(6, np.float32)], "needs a bool array"),
                          ([ok, None], "got None"), (pqv.RowMask(None, s), "needs a Searcher source")):
            before = b._where
            with pytest.raises(pqv.PqvError, match=text) as e:
                b.where(bad)
            assert e.value.code == -1 and b._where is before
    s._h = other._h = None
