"""Predicate columns, the part that needs no GPU: a table builder's corpus-aligned column is refused, before anything is
uploaded, where its files disagree on the column's type or a file's column is not as long as its index; bool operands; the
searcher's own column table."""
import numpy as np
import pytest


def _fake_table(pqv, row_base, n_rows, corpus_rows):
    class Corpus:
        rows, device = corpus_rows, 0

    s = object.__new__(pqv.TableSearcher)        # no device here: the refusals must come before any upload
    s._h, s._corpus, s._columns, s._owned_columns = None, Corpus(), {}, []
    s.row_base, s.n_rows = np.array(row_base, np.uint64), np.array(n_rows, np.uint64)
    return s


def _write(path, **columns):
    import pyarrow as pa
    import pyarrow.parquet as pq
    pq.write_table(pa.table(columns), str(path))
    return str(path)


def test_table_columns_must_have_one_type_and_the_index_rows(tmp_path):
    import pyarrow as pa
    import pq_vector_amd as pqv
    from pq_vector_amd import api
    a = _write(tmp_path / "a.parquet", id=pa.array([1, 2, 3], pa.int32()), tag=pa.array([1, 2, 3], pa.int16()))
    b = _write(tmp_path / "b.parquet", id=pa.array([4, 5], pa.int64()), tag=pa.array([4, 5], pa.int32()))
    s = _fake_table(pqv, [0, 5], [3, 2], 7)
    with pytest.raises(pqv.PqvError, match=r"column 'id' is int64 in file 1 and int32 in file 0: a table's predicate columns must have one type") as e:
        api._attach_table_columns(s, [a, b], ["id"])
    assert e.value.code == -1 and s.columns == {}
    # int16 and int32 are both resident as I32: no type refusal; the next check is the row count of file 1
    s = _fake_table(pqv, [0, 5], [3, 4], 9)
    with pytest.raises(pqv.PqvError, match=r"column 'tag' of file 1 has 2 rows, its index has 4"):
        api._attach_table_columns(s, [a, b], ["tag"])
    assert s.columns == {}
    with pytest.raises(pqv.PqvError, match="no column named 'nope'"):
        api._attach_table_columns(s, [a, b], ["nope"])
    s._h = None


def test_bool_operands_are_zero_and_one_on_integer_columns():
    import pq_vector_amd as pqv
    from pq_vector_amd import _ffi
    c = pqv.col
    for dtype in (_ffi.PQV_COL_I32, _ffi.PQV_COL_I64):
        comp = ((c("flag") == True) | (c("flag") != np.bool_(False))).compile({"flag": dtype})      # noqa: E712
        assert comp.operands.tolist() == [1, 0, 0, 0] and comp.ops.tolist() == [_ffi.PQV_OP_EQ, _ffi.PQV_OP_NE]
        assert c("flag").isin([False, True]).compile({"flag": dtype}).operands.tolist() == [0, 0, 1, 0]
    with pytest.raises(ValueError, match="float column"):
        (c("x") == True).compile({"x": _ffi.PQV_COL_F64})                                           # noqa: E712


def test_documented_mask_leaf_spelling():
    """`&` binds tighter than `<`: the comparison is parenthesised, as the module's example has it."""
    import pq_vector_amd as pqv
    from pq_vector_amd import predicate

    class Mask:
        _h, _searcher = 1, None

    assert '(pqv.col("id") < 100) & pqv.allowed(mask)' in predicate.__doc__
    m = Mask()
    comp = ((pqv.col("id") < 100) & pqv.allowed(m)).compile({"id": 0})
    assert comp.leaves == ["id", m] and comp.program == bytes([0, 1, 0x80])
    with pytest.raises(TypeError):
        pqv.col("id") < 100 & pqv.allowed(m)
