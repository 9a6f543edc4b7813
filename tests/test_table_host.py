"""Table searchers, host side: the ABI surface (header, ctypes table, Rust externs), the argument checks that TableSearcher,
searcher_for_parquet_files and the table builders make before any device use, and split_rows on hand-made row bases."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from pq_vector_amd import _ffi
    return _ffi.lib()


class _HostCorpus:
    """Stands in for a Corpus: the checks read only its shape."""

    def __init__(self, rows, dim):
        self.rows, self.dim, self._h = rows, dim, None


def _index(dim, n_clusters, n_rows):
    import pq_vector_amd as pqv
    rng = np.random.default_rng(n_rows)
    rows = np.arange(n_rows, dtype=np.uint32)
    lists = [rows[c::n_clusters] for c in range(n_clusters)]
    return pqv.Index.from_parts(dim, rng.random((n_clusters, dim), dtype=np.float32), lists)


def test_table_symbols_in_header_ffi_and_sys_rs(lib):
    from pq_vector_amd import _ffi
    header = open(os.path.join(ROOT, "include", "pqv.h")).read()
    sys_rs = open(os.path.join(ROOT, "bindings", "rust", "src", "sys.rs")).read()
    for name in ("pqv_table_searcher_create", "pqv_searcher_files"):
        assert name in _ffi.SIGNATURES
        assert getattr(lib, name).argtypes == _ffi.SIGNATURES[name][1]
        assert re.search(r"\b%s\s*\(" % name, header)
        assert re.search(r"pub fn %s\(" % name, sys_rs)
    assert "pub struct TableSearcher" in open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    assert lib.pqv_abi_version() == 101


def test_table_c_abi_rejects_null_arguments(lib):
    from pq_vector_amd import _ffi
    out = _ffi.vp()
    rc = lib.pqv_table_searcher_create(None, 1, None, None, 0, C.byref(out))
    assert rc == _ffi.PQV_ERR_INVALID and b"must not be NULL" in lib.pqv_last_error()
    rc = lib.pqv_searcher_files(None, None, None, None)
    assert rc == _ffi.PQV_ERR_INVALID and b"searcher must not be NULL" in lib.pqv_last_error()


def test_table_searcher_validates_before_device_use():
    import pq_vector_amd as pqv
    a, b = _index(8, 4, 100), _index(8, 3, 50)
    corpus = _HostCorpus(150, 8)
    with pytest.raises(pqv.PqvError, match="at least one indexed file"):
        pqv.TableSearcher([], corpus, [])
    with pytest.raises(pqv.PqvError, match="dimension 16 of file 1 does not match dimension 8 of file 0"):
        pqv.TableSearcher([a, _index(16, 2, 50)], corpus, [0, 100])
    with pytest.raises(pqv.PqvError, match="does not match corpus dimension 16"):
        pqv.TableSearcher([a, b], _HostCorpus(150, 16), [0, 100])
    with pytest.raises(pqv.PqvError, match="inside the rows of the files before it"):
        pqv.TableSearcher([a, b], corpus, [0, 99])
    with pytest.raises(pqv.PqvError, match="inside the rows of the files before it"):
        pqv.TableSearcher([a, b], _HostCorpus(400, 8), [200, 0])
    with pytest.raises(pqv.PqvError, match=r"row range \[101, 151\) of file 1 lies outside the corpus of 150 rows"):
        pqv.TableSearcher([a, b], corpus, [0, 101])
    with pytest.raises(pqv.PqvError, match="row_base has 1 entries for 2 files"):
        pqv.TableSearcher([a, b], corpus, [0])
    # every check passed: the library is reached, and (a stand-in corpus has no handle) refuses it before any device use
    with pytest.raises(pqv.PqvError, match="must not be NULL"):
        pqv.TableSearcher([a, b], corpus, [0, 100])


def test_searcher_for_parquet_files_rejects_no_files():
    import pq_vector_amd as pqv
    with pytest.raises(pqv.PqvError, match="at least one indexed file"):
        pqv.searcher_for_parquet_files([])


def test_table_builders_validation():
    import pq_vector_amd as pqv
    for n in ("TableTopkBuilder", "TableRangeBuilder", "TableSearcher", "TableSearchResult", "searcher_for_parquet_files"):
        assert n in pqv.__all__
    q = np.zeros(4, np.float32)
    files = ["/nonexistent/a.parquet", "/nonexistent/b.parquet"]
    with pytest.raises(pqv.PqvError, match="at least one indexed file"):
        pqv.TableTopkBuilder([], q)
    with pytest.raises(pqv.PqvError, match="at least one indexed file"):
        pqv.TableRangeBuilder([], q)
    with pytest.raises(pqv.PqvError, match="k must be set"):
        pqv.TableTopkBuilder(files, q).nprobe(2).search()
    with pytest.raises(pqv.PqvError, match="nprobe must be set"):
        pqv.TableTopkBuilder(files, q).k(3).search()
    with pytest.raises(pqv.PqvError, match="k must be > 0"):
        pqv.TableTopkBuilder(files, q).k(0)
    with pytest.raises(pqv.PqvError, match="nprobe must be > 0"):
        pqv.TableTopkBuilder(files, q).nprobe(0)
    with pytest.raises(pqv.PqvError, match="radius must be set"):
        pqv.TableRangeBuilder(files, q).nprobe(2).search()
    with pytest.raises(pqv.PqvError, match="nprobe must be set"):
        pqv.TableRangeBuilder(files, q).radius(1.0).search()
    with pytest.raises(pqv.PqvError, match="nprobe must be > 0"):
        pqv.TableRangeBuilder(files, q).radius(1.0).nprobe(0)
    with pytest.raises(pqv.PqvError, match="radius must not be NaN"):
        pqv.TableRangeBuilder(files, q).radius(float("nan"))


def test_split_rows_on_hand_made_row_bases():
    import pq_vector_amd as pqv
    row_base = np.array([0, 10, 25, 25, 40], dtype=np.uint64)       # file 3 is empty
    n_rows = np.array([10, 15, 0, 5, 7], dtype=np.uint64)
    rows = np.array([0, 9, 10, 24, 25, 29, 30, 39, 40, 46, 47, 0xFFFFFFFF], dtype=np.uint32)
    f, local = pqv.split_table_rows(rows, row_base, n_rows)
    assert f.tolist() == [0, 0, 1, 1, 3, 3, -1, -1, 4, 4, -1, -1]
    assert local.tolist() == [0, 9, 0, 14, 0, 4, 0xFFFFFFFF, 0xFFFFFFFF, 0, 6, 0xFFFFFFFF, 0xFFFFFFFF]
    s = object.__new__(pqv.TableSearcher)        # split_rows is host arithmetic on the searcher's row bases
    s.row_base, s.n_rows = row_base, n_rows
    f2, local2 = s.split_rows(rows)
    assert (f2 == f).all() and (local2 == local).all()
    # without row counts a file runs up to the next file's base
    f3, local3 = pqv.split_table_rows([5, 12, 100], [0, 10])
    assert f3.tolist() == [0, 1, 1] and local3.tolist() == [5, 2, 90]


def test_split_rows_by_extents_larger_than_the_row_counts():
    """A file that had rows removed keeps its ids: its extent is its index' row bound, above its count of list rows, and a
    surviving row with a local id at or above the count still belongs to the file."""
    import pq_vector_amd as pqv
    row_base = np.array([0, 100, 260], dtype=np.uint64)
    n_rows = np.array([100, 90, 40], dtype=np.uint64)          # list rows: file 1 lost 70 of its 160 ids, file 2 lost 10 of 50
    extents = np.array([100, 160, 50], dtype=np.uint64)
    rows = np.array([99, 100, 189, 190, 259, 260, 299, 300, 309, 310, 0xFFFFFFFF], dtype=np.uint32)
    f, local = pqv.split_table_rows(rows, row_base, extents)
    assert f.tolist() == [0, 1, 1, 1, 1, 2, 2, 2, 2, -1, -1]
    assert local.tolist() == [99, 0, 89, 90, 159, 0, 39, 40, 49, 0xFFFFFFFF, 0xFFFFFFFF]
    # ... which the row counts would have lost
    f_n, _ = pqv.split_table_rows(rows, row_base, n_rows)
    assert f_n.tolist() == [0, 1, 1, -1, -1, 2, 2, -1, -1, -1, -1]
    s = object.__new__(pqv.TableSearcher)        # split_rows goes by the extents where the searcher has them
    s.row_base, s.n_rows, s.extents = row_base, n_rows, extents
    f2, local2 = s.split_rows(rows)
    assert (f2 == f).all() and (local2 == local).all()


def test_table_args_take_the_row_bound_as_a_files_extent():
    import pq_vector_amd as pqv
    rows = np.arange(1, 100, 2, dtype=np.uint32)                       # what a remove of the even ids leaves: 50 rows, ids up to 99
    rng = np.random.default_rng(0)
    holes = pqv.Index.from_parts(8, rng.random((2, 8), dtype=np.float32), [rows[:20], rows[20:]])
    assert holes.n_rows == 50 and holes.row_bound == 100
    b = _index(8, 3, 50)
    with pytest.raises(pqv.PqvError, match=r"row range of file 1 starts at 50, inside the rows of the files before it"):
        pqv.TableSearcher([holes, b], _HostCorpus(150, 8), [0, 50])
    with pytest.raises(pqv.PqvError, match=r"row range \[60, 160\) of file 1 lies outside the corpus of 150 rows"):
        pqv.TableSearcher([b, holes], _HostCorpus(150, 8), [0, 60])
    with pytest.raises(pqv.PqvError, match="must not be NULL"):        # every check passed: spaced by the bound
        pqv.TableSearcher([holes, b], _HostCorpus(150, 8), [0, 100])


def test_parquet_table_paths_take_a_files_extent(tmp_path, monkeypatch):
    """A table of Parquet files after a DELETE: file 1 has four rows, its index' lists hold two of them.  The predicate columns and
    the per-file where() arrays cover the file's rows -- its extent --, not its count of list rows."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    import pq_vector_amd as pqv
    from pq_vector_amd import api
    paths = []
    for f, tags in enumerate(([1, 2, 3], [4, None, 6, 7])):
        paths.append(str(tmp_path / f"{f}.parquet"))
        pq.write_table(pa.table({"tag": pa.array(tags, pa.int32())}), paths[-1])

    class Corpus:
        rows, device = 9, 0

    class Stub(api.Column):          # no device here: what would be uploaded is kept instead
        def close(self):
            self._h = None

    uploaded = {}

    def upload(values, valid=None, device=0):
        uploaded.update(values=np.asarray(values).copy(), valid=np.asarray(valid).copy())
        return Stub(object())
    monkeypatch.setattr(api.Column, "upload", staticmethod(upload))
    s = object.__new__(pqv.TableSearcher)
    s._h, s._corpus, s._columns, s._owned_columns = None, Corpus(), {}, []
    s.row_base, s.n_rows = np.array([0, 5], np.uint64), np.array([3, 2], np.uint64)
    with pytest.raises(pqv.PqvError, match="column 'tag' of file 1 has 4 rows, its index has 2"):          # by the list rows: refused
        api._attach_table_columns(s, paths, ["tag"])
    s.extents = [3, 4]
    api._attach_table_columns(s, paths, ["tag"])
    assert uploaded["values"].tolist() == [1, 2, 3, 0, 0, 4, 0, 6, 7] and uploaded["valid"].tolist() == [1, 1, 1, 0, 0, 1, 0, 1, 1]
    s.row_mask = lambda allowed: np.asarray(allowed).copy()
    per_file = [np.array([True, False, True]), np.array([False, True, True, True])]
    assert api._resolve_table_where(per_file, paths, s).tolist() == [1, 0, 1, 0, 0, 0, 1, 1, 1]
    with pytest.raises(pqv.PqvError, match="row mask has 2 rows, the corpus has 4"):
        api._resolve_table_where([per_file[0], per_file[1][:2]], paths, s)


def test_index_row_bound_in_header_ffi_and_sys_rs(lib):
    import pq_vector_amd as pqv
    from pq_vector_amd import _ffi
    assert "pqv_index_row_bound" in _ffi.SIGNATURES
    assert re.search(r"\bpqv_index_row_bound\s*\(", open(os.path.join(ROOT, "include", "pqv.h")).read())
    assert "pub fn pqv_index_row_bound(" in open(os.path.join(ROOT, "bindings", "rust", "src", "sys.rs")).read()
    rng = np.random.default_rng(0)
    rows = np.arange(1, 100, 2, dtype=np.uint32)
    holes = pqv.Index.from_parts(8, rng.random((2, 8), dtype=np.float32), [rows[:20], rows[20:]])
    assert lib.pqv_index_row_bound(holes._h) == 100 == holes.row_bound and lib.pqv_index_n_rows(holes._h) == 50
    empty = pqv.Index.from_parts(8, rng.random((2, 8), dtype=np.float32), [rows[:0], rows[:0]])
    assert lib.pqv_index_row_bound(empty._h) == 0 and lib.pqv_index_row_bound(None) == 0
