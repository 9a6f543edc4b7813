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
