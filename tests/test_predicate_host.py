"""Predicate masks, the part that needs no GPU: the new symbols in header / ctypes table / sys.rs, pqv_predicate_check, the
argument checks that come before device use, and the Python compiler (pq_vector_amd.predicate) -- its compiled programs,
evaluated by tests/predicate_ref.py, against pyarrow's evaluation of the independently translated tree."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import predicate_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["pqv_column_upload", "pqv_column_from_device", "pqv_column_rows", "pqv_column_dtype", "pqv_column_device",
               "pqv_column_free", "pqv_predicate_check", "pqv_row_mask_from_predicates", "pqv_row_mask_to_bytes"]


@pytest.fixture(scope="module")
def lib():
    from pq_vector_amd import _ffi
    return _ffi.lib()


def test_predicate_symbols_exported_bound_and_in_sys_rs(lib):
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
    assert "typedef struct pqv_column pqv_column;" in hdr and "pub struct PqvColumn" in sys_rs
    for macro, value in (("PQV_COL_I32", 0), ("PQV_COL_I64", 1), ("PQV_COL_F32", 2), ("PQV_COL_F64", 3), ("PQV_OP_EQ", 0),
                         ("PQV_OP_NE", 1), ("PQV_OP_LT", 2), ("PQV_OP_LE", 3), ("PQV_OP_GT", 4), ("PQV_OP_GE", 5),
                         ("PQV_OP_BETWEEN", 6), ("PQV_OP_IS_NULL", 7), ("PQV_OP_MASK", 8), ("PQV_OP_NOT", 0x100),
                         ("PQV_PRED_AND", 0x80), ("PQV_PRED_OR", 0x81)):
        m = re.search(r"#define\s+%s\s+(\w+)" % macro, hdr)
        assert m and int(m.group(1), 0) == value == getattr(_ffi, macro), macro
        assert re.search(r"pub const %s: \w+ = (0x)?%x;" % (macro, value), sys_rs), macro
    for f, needle in (("bindings/rust/src/lib.rs", "pub struct Column"), ("bindings/rust/src/lib.rs", "impl Drop for Column"),
                      ("bindings/rust/src/lib.rs", "pub fn from_predicates"), ("pq-vector_amd/host/pqv.hpp", "class Column"),
                      ("pq-vector_amd/host/pqv.hpp", "from_predicates")):
        assert needle in open(os.path.join(ROOT, f)).read(), (f, needle)
    assert lib.pqv_abi_version() == 101


def _check(lib, program, n_leaves):
    buf = (C.c_uint8 * max(1, len(program)))(*program)
    depth = C.c_uint32(99)
    rc = lib.pqv_predicate_check(buf, len(program), n_leaves, C.byref(depth))
    return rc, depth.value, lib.pqv_last_error().decode()


def test_predicate_check_accepts_and_rejects(lib):
    AND, OR = 0x80, 0x81
    assert _check(lib, [0], 1)[:2] == (0, 1)
    assert _check(lib, [0, 1, AND], 2)[:2] == (0, 2)
    assert _check(lib, [0, 1, AND, 2, OR], 3)[:2] == (0, 2)
    assert _check(lib, [0, 1, 2, OR, AND], 3)[:2] == (0, 3)
    assert _check(lib, [0, 0, OR], 1)[:2] == (0, 2)                            # a leaf may be pushed twice
    # right-nested over 32 leaves: depth 32, 63 bytes -- the largest program
    deep = list(range(32)) + [AND] * 31
    assert len(deep) == 63 and _check(lib, deep, 32)[:2] == (0, 32)
    left = [0] + [x for i in range(1, 32) for x in (i, OR)]
    assert len(left) == 63 and _check(lib, left, 32)[:2] == (0, 2)

    def refused(program, n_leaves, text):
        rc, depth, err = _check(lib, program, n_leaves)
        assert rc == -1 and depth == 0 and text in err, (program, err)
    refused([], 1, "predicate program is empty")
    refused([AND], 1, "predicate program is malformed")                       # underflow
    refused([0, AND], 1, "predicate program is malformed")
    refused([0, 1], 2, "predicate program is malformed")                      # two values left
    refused([0, 1, AND, OR], 2, "predicate program is malformed")
    refused([0, 0x40, AND], 2, "predicate program is malformed")              # unknown byte
    refused([0, 0x82, AND], 2, "predicate program is malformed")
    refused([0, 2, AND], 2, "predicate program is malformed")                 # leaf index >= n_leaves
    refused([0, 1, AND], 33, "predicate has 33 leaves, at most 32")
    refused([0] * 33 + [AND] * 32, 1, "predicate program is malformed")       # 65 bytes, depth 33
    refused([0, 0, AND] + [0, AND] * 31, 1, "predicate program is malformed")  # 65 bytes
    # max_depth may be NULL
    buf = (C.c_uint8 * 3)(0, 1, OR)
    assert lib.pqv_predicate_check(buf, 3, 2, None) == 0
    assert lib.pqv_predicate_check(None, 3, 2, None) == -1 and b"program must not be NULL" in lib.pqv_last_error()


def test_predicate_c_abi_validates_before_device_use(lib):
    inv = -1
    h = C.c_void_p()
    vals = (C.c_int32 * 4)()
    assert lib.pqv_column_upload(0, 0, vals, None, 4, None) == inv and b"out must not be NULL" in lib.pqv_last_error()
    assert lib.pqv_column_upload(0, 4, vals, None, 4, C.byref(h)) == inv and b"unknown column type" in lib.pqv_last_error()
    assert lib.pqv_column_upload(0, -1, vals, None, 4, C.byref(h)) == inv and b"unknown column type" in lib.pqv_last_error()
    assert lib.pqv_column_upload(0, 0, None, None, 4, C.byref(h)) == inv and b"values must not be NULL" in lib.pqv_last_error()
    assert lib.pqv_column_from_device(0, 9, None, None, 4, C.byref(h)) == inv and b"unknown column type" in lib.pqv_last_error()
    assert lib.pqv_column_from_device(0, 1, None, None, 4, C.byref(h)) == inv and b"d_values must not be NULL" in lib.pqv_last_error()
    assert lib.pqv_column_from_device(0, 1, None, None, 4, None) == inv and b"out must not be NULL" in lib.pqv_last_error()
    assert h.value is None
    assert lib.pqv_column_rows(None) == 0 and lib.pqv_column_dtype(None) == -1 and lib.pqv_column_device(None) == -1
    lib.pqv_column_free(None)

    prog = (C.c_uint8 * 1)(0)
    ops = (C.c_uint32 * 1)(5)
    operands = (C.c_uint64 * 2)(2, 0)
    cols = (C.c_void_p * 1)(None)
    fake = C.c_void_p(8)          # never dereferenced: the checks below come first
    f = lib.pqv_row_mask_from_predicates
    assert f(None, 1, cols, None, ops, operands, prog, 1, None, None) == inv and b"out must not be NULL" in lib.pqv_last_error()
    assert f(None, 1, cols, None, ops, operands, prog, 1, None, C.byref(h)) == inv and b"searcher must not be NULL" in lib.pqv_last_error()
    assert f(fake, 1, cols, None, ops, operands, prog, 0, None, C.byref(h)) == inv and b"predicate program is empty" in lib.pqv_last_error()
    assert f(fake, 33, cols, None, ops, operands, prog, 1, None, C.byref(h)) == inv and b"predicate has 33 leaves, at most 32" in lib.pqv_last_error()
    bad = (C.c_uint8 * 2)(0, 0x80)
    assert f(fake, 1, cols, None, ops, operands, bad, 2, None, C.byref(h)) == inv and b"predicate program is malformed" in lib.pqv_last_error()
    assert f(fake, 1, cols, None, None, operands, prog, 1, None, C.byref(h)) == inv and b"ops must not be NULL" in lib.pqv_last_error()
    assert f(fake, 1, cols, None, ops, None, prog, 1, None, C.byref(h)) == inv and b"operands must not be NULL" in lib.pqv_last_error()
    assert h.value is None

    out = (C.c_uint8 * 4)()
    assert lib.pqv_row_mask_to_bytes(None, out, 4) == inv and b"row mask must not be NULL" in lib.pqv_last_error()


def test_compiled_random_trees_equal_pyarrow():
    columns = ref.make_columns(257, seed=11)
    table = ref.arrow_table(columns)
    trees = ref.compilable_trees(300, columns, depth=4, seed=5)
    n_true = 0
    for p, comp in trees:
        assert len(comp.leaves) <= 32 and len(comp.program) <= 63
        assert all(int(op) & 0xFF != 8 for op in comp.ops)
        got = ref.evaluate(comp, columns)
        want = ref.evaluate_arrow(p, columns, table)
        assert (got == want).all(), (comp, np.flatnonzero(got != want)[:5])
        n_true += int(got.sum())
    assert 0 < n_true < 300 * 257           # the trees are neither all-false nor all-true


def test_compile_pushes_not_to_the_leaves_and_shares_equal_leaves():
    from pq_vector_amd import _ffi, predicate
    c = predicate.col
    comp = predicate.compile(~((c("a") >= 2) & (c("b") < 1.5)), {"a": _ffi.PQV_COL_I64, "b": _ffi.PQV_COL_F32})
    assert comp.leaves == ["a", "b"] and comp.program == bytes([0, 1, _ffi.PQV_PRED_OR])
    assert comp.ops.tolist() == [_ffi.PQV_OP_GE | _ffi.PQV_OP_NOT, _ffi.PQV_OP_LT | _ffi.PQV_OP_NOT]
    assert comp.operands.tolist() == [2, 0, np.float64(1.5).view(np.uint64), 0]
    comp = predicate.compile(~~(c("a") == -1) | (c("a") == -1), {"a": _ffi.PQV_COL_I32})
    assert comp.leaves == ["a"] and comp.program == bytes([0, 0, _ffi.PQV_PRED_OR]) and comp.operands[0] == 2**64 - 1
    comp = predicate.compile(c("a").between(1, 3) & ~c("a").is_null(), {"a": _ffi.PQV_COL_I32})
    assert comp.ops.tolist() == [_ffi.PQV_OP_BETWEEN, _ffi.PQV_OP_IS_NULL | _ffi.PQV_OP_NOT] and comp.operands.tolist() == [1, 3, 0, 0]
    assert ((c("a") > 1) | (c("b") > 1) & (c("a") < 0)).columns() == ["a", "b"]
    with pytest.raises(TypeError):
        bool(c("a") > 1)
    with pytest.raises(KeyError):
        predicate.compile(c("nope") > 1, {"a": 0})


def test_operand_conversion_errors():
    from pq_vector_amd import _ffi, predicate
    c = predicate.col
    ints = {"x": _ffi.PQV_COL_I32, "y": _ffi.PQV_COL_I64}
    floats = {"x": _ffi.PQV_COL_F32, "y": _ffi.PQV_COL_F64}
    for bad in (1.5, float("nan"), float("inf"), "3", None, 2**63, -2**63 - 1):
        for name in ints:
            with pytest.raises(ValueError):
                predicate.compile(c(name) == bad, ints)
    with pytest.raises(ValueError):
        predicate.compile(c("y").between(0, 2.5), ints)
    # exact conversions pass: integral floats, numpy scalars, the int64 extremes, beyond-int32 on an I32 column
    for good in (3.0, np.int32(7), np.int64(-2**63), 2**63 - 1, 2**40, np.float32(4.0)):
        comp = predicate.compile(c("x") == good, ints)
        assert comp.operands[0] == np.int64(int(good)).view(np.uint64)
    for bad in (2**53 + 1, -2**53 - 1, "1.0", None):
        for name in floats:
            with pytest.raises(ValueError):
                predicate.compile(c(name) < bad, floats)
    for good in (2**53, -2**53, 1, 0.1, np.float32(0.1), float("nan"), float("-inf")):
        comp = predicate.compile(c("y") < good, floats)
        assert comp.operands[0] == np.float64(good).view(np.uint64)
    with pytest.raises(ValueError, match="NaN"):
        predicate.compile(c("y").isin([1.0, float("nan")]), floats)
    with pytest.raises(ValueError):
        c("y").isin([])
    # 33 distinct leaves
    p = c("y") == 0
    for i in range(1, 33):
        p = p | (c("y") == i)
    with pytest.raises(ValueError, match="more than 32 leaves"):
        predicate.compile(p, ints)
    p = c("y").isin(range(32))
    assert len(predicate.compile(p, ints).leaves) == 32
    # a right-nested AND of 32 leaves: depth 32, the limit
    p = c("y") != 31
    for i in range(30, -1, -1):
        p = (c("y") != i) & p
    comp = predicate.compile(p, ints)
    assert len(comp.program) == 63 and comp.program[:32] == bytes(range(32))


def test_not_in_drops_null_rows_where_arrow_invert_is_in_keeps_them():
    import pyarrow as pa
    import pyarrow.compute as pc
    from pq_vector_amd import predicate
    values = np.array([1, 2, 3, 0, 2], dtype=np.int64)
    valid = np.array([1, 1, 1, 0, 1], dtype=np.uint8)
    columns = {"v": (values, valid)}
    p = ~predicate.col("v").isin([2, 9])
    comp = predicate.compile(p, ref.dtypes_of(columns))
    got = ref.evaluate(comp, columns)
    assert got.tolist() == [1, 0, 1, 0, 0]                         # SQL's NOT IN: the NULL row is dropped
    assert (got == ref.evaluate_arrow(p, columns)).all()           # ... as Kleene logic over the EQ leaves gives
    arr = pa.array(values, mask=valid == 0)
    kept = pc.invert(pc.is_in(arr, value_set=pa.array([2, 9]))).to_numpy(zero_copy_only=False)
    assert kept.tolist() == [True, False, True, True, False]        # the deliberate difference
    assert ref.evaluate(predicate.compile(predicate.col("v").isin([2, 9]), ref.dtypes_of(columns)), columns).tolist() == [0, 1, 0, 0, 1]


def test_scalar_arrays_type_map_and_refusals(tmp_path):
    import datetime
    import pyarrow as pa
    import pyarrow.parquet as pq
    import pq_vector_amd as pqv
    from pq_vector_amd import _ffi, parquet_io
    from pq_vector_amd.api import scalar_arrays
    cases = [(pa.int8(), [1, None, -3], np.int32), (pa.int16(), [1, None, -3], np.int32), (pa.uint8(), [1, None, 200], np.int32),
             (pa.uint16(), [1, None, 65535], np.int32), (pa.int32(), [1, None, -3], np.int32), (pa.uint32(), [1, None, 2**32 - 1], np.int64),
             (pa.int64(), [1, None, 2**53 + 1], np.int64), (pa.bool_(), [True, None, False], np.int32),
             (pa.float32(), [1.5, None, float("nan")], np.float32), (pa.float64(), [0.1, None, float("inf")], np.float64)]
    for typ, data, want in cases:
        a, v, dtype = scalar_arrays(pa.array(data, type=typ))
        assert a.dtype == want and dtype == ref.DTYPE_OF[np.dtype(want)] and v.tolist() == [1, 0, 1], typ
        assert a[0] == data[0] and (a[2] == data[2] or data[2] != data[2]), typ
    a, v, dtype = scalar_arrays(pa.chunked_array([pa.array([1, 2], type=pa.int64()), pa.array([3], type=pa.int64())]))
    assert a.tolist() == [1, 2, 3] and v is None and dtype == _ffi.PQV_COL_I64
    day = datetime.date(2024, 3, 1)
    a, v, dtype = scalar_arrays(pa.array([day, None], type=pa.date32()))
    assert dtype == _ffi.PQV_COL_I32 and a[0] == (day - datetime.date(1970, 1, 1)).days and v.tolist() == [1, 0]
    for typ in (pa.date64(), pa.timestamp("us")):
        a, v, dtype = scalar_arrays(pa.array([datetime.datetime(2024, 3, 1), None], type=typ))
        assert dtype == _ffi.PQV_COL_I64 and a.dtype == np.int64 and v.tolist() == [1, 0]
    a, v, dtype = scalar_arrays(pa.array([datetime.time(1, 2, 3), None], type=pa.time64("us")))
    assert dtype == _ffi.PQV_COL_I64 and a[0] == 3723 * 10**6
    for bad in (pa.array(["x"]), pa.array([1], type=pa.uint64()), pa.array([[1]], type=pa.list_(pa.int32()))):
        with pytest.raises(pqv.PqvError, match=r"column 'tag' has type .*pyarrow expression") as e:
            scalar_arrays(bad, name="tag")
        assert str(bad.type) in str(e.value)
    with pytest.raises(pqv.PqvError, match="int32, int64, float32 or float64"):
        scalar_arrays(np.zeros(3, np.uint8))
    with pytest.raises(pqv.PqvError, match="valid has 2 entries for 3 values"):
        scalar_arrays(np.zeros(3, np.int32), np.ones(2, bool))
    # a file's column, row groups in file order; a string column is refused by name
    path = str(tmp_path / "t.parquet")
    pq.write_table(pa.table({"id": pa.array([0, 1, None, 3, 4], type=pa.int16()), "tag": pa.array(list("abcde"))}), path, row_group_size=2)
    a, v, dtype = parquet_io.read_scalar_column(path, "id")
    assert a.tolist() == [0, 1, 0, 3, 4] and v.tolist() == [1, 1, 0, 1, 1] and dtype == _ffi.PQV_COL_I32
    a, v, _ = parquet_io.read_scalar_column(path, "id", row_groups=[1, 2])
    assert a.tolist() == [0, 3, 4] and v.tolist() == [0, 1, 1]
    with pytest.raises(pqv.PqvError, match=r"column 'tag' has type string.*pyarrow expression"):
        parquet_io.read_scalar_column(path, "tag")
    with pytest.raises(pqv.PqvError, match="no column named 'nope'"):
        parquet_io.read_scalar_column(path, "nope")


def test_where_accepts_a_predicate_on_all_four_builders_without_touching_a_device(tmp_path):
    import pq_vector_amd as pqv
    q = np.zeros(2, np.float32)
    p = pqv.col("id") >= 2
    path = str(tmp_path / "x.parquet")
    open(path, "wb").close()                      # (where() does not open the file)
    for b in (pqv.TopkBuilder(path, q), pqv.RangeBuilder(path, q), pqv.TableTopkBuilder([path, path], q),
              pqv.TableRangeBuilder([path, path], q)):
        assert b.where(p) is b and b._where is p
    for name in ("Column", "col", "allowed", "load_scalar_column"):
        assert name in pqv.__all__ and hasattr(pqv, name)
    with pytest.raises(TypeError):
        pqv.allowed(np.ones(3, bool))
