"""Reference semantics of predicate masks (pqv.h: pqv_row_mask_from_predicates), twice and independently:

  evaluate()       numpy evaluation of a COMPILED predicate (leaf table + postfix program), the header's rules spelled out;
  to_expression()  translation of the predicate TREE (before compile: NOT still in the tree) to a pyarrow expression, whose
                   Kleene evaluation followed by fill_null(False) is what SQL's WHERE keeps.

Plus the shared test data: typed columns with NULLs and the awkward values, and a seeded random tree generator."""
import struct

import numpy as np

from pq_vector_amd import _ffi, predicate

OPS = (_ffi.PQV_OP_EQ, _ffi.PQV_OP_NE, _ffi.PQV_OP_LT, _ffi.PQV_OP_LE, _ffi.PQV_OP_GT, _ffi.PQV_OP_GE, _ffi.PQV_OP_BETWEEN,
       _ffi.PQV_OP_IS_NULL)
DTYPE_OF = {np.dtype(np.int32): _ffi.PQV_COL_I32, np.dtype(np.int64): _ffi.PQV_COL_I64,
            np.dtype(np.float32): _ffi.PQV_COL_F32, np.dtype(np.float64): _ffi.PQV_COL_F64}


def _operand(bits, integer):
    raw = struct.pack("<Q", int(bits))
    return struct.unpack("<q" if integer else "<d", raw)[0]


def leaf_truth(op, a_bits, b_bits, values, valid):
    """bool [n]: valid && (cmp(x) != negate); IS_NULL: (!valid) != negate."""
    neg = bool(op & _ffi.PQV_OP_NOT)
    o = op & 0xFF
    ok = np.ones(values.shape, bool) if valid is None else np.asarray(valid) != 0
    if o == _ffi.PQV_OP_IS_NULL:
        return (~ok) != neg
    integer = values.dtype.kind == "i"
    x = values.astype(np.int64) if integer else values.astype(np.float64)
    a, b = _operand(a_bits, integer), _operand(b_bits, integer)
    a = np.int64(a) if integer else np.float64(a)
    b = np.int64(b) if integer else np.float64(b)
    with np.errstate(invalid="ignore"):
        t = {_ffi.PQV_OP_EQ: lambda: x == a, _ffi.PQV_OP_NE: lambda: x != a, _ffi.PQV_OP_LT: lambda: x < a,
             _ffi.PQV_OP_LE: lambda: x <= a, _ffi.PQV_OP_GT: lambda: x > a, _ffi.PQV_OP_GE: lambda: x >= a,
             _ffi.PQV_OP_BETWEEN: lambda: (a <= x) & (x <= b)}[o]()
    return ok & (t != neg)


def evaluate(compiled, columns, mask_bytes=None):
    """uint8 [n]: the compiled predicate over columns {name: (values, valid or None)}; MASK leaves read
    mask_bytes[id(row mask)] (uint8 [n])."""
    stack = []
    for c in compiled.program:
        if c in (_ffi.PQV_PRED_AND, _ffi.PQV_PRED_OR):
            r, l = stack.pop(), stack.pop()
            stack.append(l & r if c == _ffi.PQV_PRED_AND else l | r)
            continue
        what, op = compiled.leaves[c], int(compiled.ops[c])
        if (op & 0xFF) == _ffi.PQV_OP_MASK:
            stack.append((np.asarray(mask_bytes[id(what)]) != 0) != bool(op & _ffi.PQV_OP_NOT))
        else:
            values, valid = columns[what]
            stack.append(leaf_truth(op, compiled.operands[2 * c], compiled.operands[2 * c + 1], values, valid))
    assert len(stack) == 1
    return stack[0].astype(np.uint8)


def dtypes_of(columns):
    return {name: DTYPE_OF[values.dtype] for name, (values, _) in columns.items()}


# ---- the predicate tree -> pyarrow -----------------------------------------------------------------------------------------
def to_expression(p, columns):
    """The pyarrow.compute.Expression of a predicate tree over a table of `columns` (no MASK leaves)."""
    import pyarrow as pa
    import pyarrow.compute as pc
    if isinstance(p, predicate._Not):
        return ~to_expression(p.inner, columns)
    if isinstance(p, predicate._Bin):
        l, r = to_expression(p.left, columns), to_expression(p.right, columns)
        return (l & r) if p.kind == _ffi.PQV_PRED_AND else (l | r)
    f = pc.field(p.column)
    if p.op == _ffi.PQV_OP_IS_NULL:
        return f.is_null()
    integer = columns[p.column][0].dtype.kind == "i"

    def lit(v):
        return pa.scalar(int(v), type=pa.int64()) if integer else pa.scalar(float(v), type=pa.float64())
    if p.op == _ffi.PQV_OP_BETWEEN:
        return (f >= lit(p.lo)) & (f <= lit(p.hi))
    a = lit(p.lo)
    return {_ffi.PQV_OP_EQ: lambda: f == a, _ffi.PQV_OP_NE: lambda: f != a, _ffi.PQV_OP_LT: lambda: f < a,
            _ffi.PQV_OP_LE: lambda: f <= a, _ffi.PQV_OP_GT: lambda: f > a, _ffi.PQV_OP_GE: lambda: f >= a}[p.op]()


def arrow_table(columns):
    import pyarrow as pa
    return pa.table({name: pa.array(values, mask=None if valid is None else np.asarray(valid) == 0)
                     for name, (values, valid) in columns.items()})


def evaluate_arrow(p, columns, table=None):
    """uint8 [n]: the tree evaluated by pyarrow with Kleene logic, NULL counting as false."""
    import pyarrow.compute as pc
    import pyarrow.dataset as ds
    table = arrow_table(columns) if table is None else table
    col = ds.dataset(table).to_table(columns={"m": to_expression(p, columns)}).column("m")
    return pc.fill_null(col, False).combine_chunks().to_numpy(zero_copy_only=False).astype(np.uint8)


# ---- test data --------------------------------------------------------------------------------------------------------------
def make_columns(n, seed):
    """{name: (values, valid or None)}: i32, i64 (2^53, 2^53 + 1, values above 2^32), f32 and f64 (NaN, +-inf, -0.0), each with
    about 15 % NULLs, and `plain`, an i32 column without validity.  Small value ranges: comparisons hit often."""
    rng = np.random.default_rng(seed)
    i32 = rng.integers(-5, 6, n).astype(np.int32)
    i32[rng.integers(0, n, max(1, n // 50))] = np.int32(2**31 - 1)
    i32[rng.integers(0, n, max(1, n // 50))] = np.int32(-2**31)
    i64 = rng.integers(-5, 6, n).astype(np.int64)
    special = np.array([2**53, 2**53 + 1, 2**32 + 7, -(2**40), 2**63 - 1, -(2**63)], dtype=np.int64)
    where = rng.integers(0, n, max(6, n // 8))
    i64[where] = special[rng.integers(0, len(special), where.size)]
    f32 = (rng.integers(-8, 9, n) * 0.5).astype(np.float32)
    f64 = (rng.integers(-8, 9, n) * 0.25).astype(np.float64)
    for arr in (f32, f64):
        where = rng.integers(0, n, max(4, n // 8))
        arr[where] = np.array([np.nan, np.inf, -np.inf, -0.0], dtype=arr.dtype)[rng.integers(0, 4, where.size)]
    f64[rng.integers(0, n, max(1, n // 50))] = 0.1
    plain = rng.integers(0, 4, n).astype(np.int32)

    def nulls():
        return (rng.random(n) >= 0.15).astype(np.uint8)
    return {"i32": (i32, nulls()), "i64": (i64, nulls()), "f32": (f32, nulls()), "f64": (f64, nulls()), "plain": (plain, None)}


def _pick_operand(rng, values, member=False):
    """An operand for a column: mostly one of its own values (so that EQ hits), which converts exactly by construction."""
    v = values[rng.integers(0, len(values))]
    if values.dtype.kind == "i":
        return int(v) if rng.random() < 0.8 else int(rng.integers(-6, 7))
    v = float(v) if rng.random() < 0.8 else float(rng.integers(-8, 9)) * 0.5
    if member and v != v:
        v = 0.5
    return v


def random_leaf(rng, columns):
    name = list(columns)[rng.integers(0, len(columns))]
    values = columns[name][0]
    c = predicate.col(name)
    kind = rng.integers(0, 10)
    if kind == 8:
        return c.is_null()
    if kind == 9:
        return c.isin([_pick_operand(rng, values, member=True) for _ in range(int(rng.integers(1, 4)))])
    if kind == 6 or kind == 7:
        lo, hi = _pick_operand(rng, values), _pick_operand(rng, values)
        if lo == lo and hi == hi and lo > hi:
            lo, hi = hi, lo
        return c.between(lo, hi)
    a = _pick_operand(rng, values)
    return (c == a, c != a, c < a, c <= a, c > a, c >= a)[kind]


def random_tree(rng, columns, depth):
    """A random predicate of at most `depth` levels of & / | over random leaves, ~ sprinkled at every level."""
    if depth == 0 or rng.random() < 0.25:
        p = random_leaf(rng, columns)
    else:
        l, r = random_tree(rng, columns, depth - 1), random_tree(rng, columns, depth - 1)
        p = (l & r) if rng.random() < 0.5 else (l | r)
    return ~p if rng.random() < 0.3 else p


def compilable_trees(count, columns, depth, seed):
    """`count` seeded random trees that fit the limits (32 leaves, 63 program bytes), with their compiled form."""
    rng = np.random.default_rng(seed)
    dt = dtypes_of(columns)
    out = []
    while len(out) < count:
        p = random_tree(rng, columns, depth)
        try:
            out.append((p, predicate.compile(p, dt)))
        except ValueError as e:
            assert "leaves" in str(e) or "program" in str(e), e
    return out
