"""Predicates over resident scalar columns (pqv.h: pqv_row_mask_from_predicates): a small expression class and its compiler.

    pqv.col("id") >= 2
    (pqv.col("price").between(10, 20) | pqv.col("tag").isin([3, 5])) & ~pqv.col("deleted_at").is_null()
    (pqv.col("id") < 100) & pqv.allowed(mask)        # an existing RowMask of the same searcher as a leaf

compile() turns such a tree into what the C entry point takes -- a leaf table (column names / row masks, ops, operand bits) and
a postfix program -- with NOT pushed down to the leaves (De Morgan), since the device interpreter has AND and OR only.  Host-only:
nothing here touches the library or a device.
"""
import math
import struct
from collections import namedtuple

import numpy as np

from . import _ffi

Compiled = namedtuple("Compiled", "leaves ops operands program")
Compiled.__doc__ = """leaves: per leaf a column name (str) or, for a MASK leaf, the RowMask; ops: uint32 [n] (PQV_OP_* | PQV_OP_NOT);
operands: uint64 [2 n] (int64 bits for integer columns, double bits for float columns); program: postfix bytes."""

MAX_LEAVES = 32
MAX_PROGRAM = 63
MAX_DEPTH = 32

_INT_TYPES = (_ffi.PQV_COL_I32, _ffi.PQV_COL_I64)
_FLOAT_TYPES = (_ffi.PQV_COL_F32, _ffi.PQV_COL_F64)


class Predicate:
    """A boolean expression over columns; combine with & | ~ (Python's `and` / `or` / `not` do not work on it)."""

    def __and__(self, other):
        return _Bin(_ffi.PQV_PRED_AND, self, _as_predicate(other))

    def __or__(self, other):
        return _Bin(_ffi.PQV_PRED_OR, self, _as_predicate(other))

    def __invert__(self):
        return _Not(self)

    def __bool__(self):
        raise TypeError("a predicate has no truth value: combine predicates with & | ~")

    def columns(self):
        """The column names the predicate reads, in first-use order."""
        out = []
        for leaf in _leaves(self):
            if leaf.column is not None and leaf.column not in out:
                out.append(leaf.column)
        return out

    def compile(self, dtypes):
        return compile(self, dtypes)


def _as_predicate(x):
    if not isinstance(x, Predicate):
        raise TypeError(f"a predicate combines with predicates, got {type(x).__name__}")
    return x


class _Leaf(Predicate):
    def __init__(self, column, op, lo=None, hi=None, mask=None, member=False):
        self.column, self.op, self.lo, self.hi, self.mask, self.member = column, op, lo, hi, mask, member

    def __repr__(self):
        return f"Leaf({self.column if self.mask is None else 'mask'}, op={self.op}, {self.lo!r}, {self.hi!r})"


class _Bin(Predicate):
    def __init__(self, kind, left, right):
        self.kind, self.left, self.right = kind, left, right


class _Not(Predicate):
    def __init__(self, inner):
        self.inner = inner


def _leaves(p):
    if isinstance(p, _Leaf):
        yield p
    elif isinstance(p, _Not):
        yield from _leaves(p.inner)
    else:
        yield from _leaves(p.left)
        yield from _leaves(p.right)


class ColumnRef:
    """pqv.col(name): comparisons against Python / numpy scalars give predicates."""
    __hash__ = None

    def __init__(self, name):
        if not isinstance(name, str) or not name:
            raise TypeError("col() needs a column name")
        self.name = name

    def __eq__(self, v):
        return _Leaf(self.name, _ffi.PQV_OP_EQ, v)

    def __ne__(self, v):
        return _Leaf(self.name, _ffi.PQV_OP_NE, v)

    def __lt__(self, v):
        return _Leaf(self.name, _ffi.PQV_OP_LT, v)

    def __le__(self, v):
        return _Leaf(self.name, _ffi.PQV_OP_LE, v)

    def __gt__(self, v):
        return _Leaf(self.name, _ffi.PQV_OP_GT, v)

    def __ge__(self, v):
        return _Leaf(self.name, _ffi.PQV_OP_GE, v)

    def between(self, lo, hi):
        """lo <= x <= hi"""
        return _Leaf(self.name, _ffi.PQV_OP_BETWEEN, lo, hi)

    def is_null(self):
        return _Leaf(self.name, _ffi.PQV_OP_IS_NULL)

    def isin(self, values):
        """x equals one of `values` (an OR of EQ leaves).  Negated it drops NULL rows, as SQL's NOT IN does."""
        values = list(values)
        if not values:
            raise ValueError("isin() needs at least one value")
        out = None
        for v in values:
            leaf = _Leaf(self.name, _ffi.PQV_OP_EQ, v, member=True)
            out = leaf if out is None else _Bin(_ffi.PQV_PRED_OR, out, leaf)
        return out


def col(name):
    return ColumnRef(name)


def allowed(row_mask):
    """An existing RowMask of the same searcher as a leaf (PQV_OP_MASK): true where the mask allows the row."""
    if not hasattr(row_mask, "_h") or not hasattr(row_mask, "_searcher"):
        raise TypeError(f"allowed() needs a RowMask, got {type(row_mask).__name__}")
    return _Leaf(None, _ffi.PQV_OP_MASK, mask=row_mask)


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _is_float(v):
    return isinstance(v, (float, np.floating))


def _operand_bits(v, dtype, column, member):
    """The 64 operand bits of scalar v for a column of dtype; ValueError where v does not convert exactly."""
    if dtype in _INT_TYPES:
        if isinstance(v, (bool, np.bool_)):          # (a Parquet bool column is resident as I32 0 / 1)
            v = int(v)
        if _is_float(v) and math.isfinite(float(v)) and float(v).is_integer():
            v = int(v)
        if not _is_int(v):
            raise ValueError(f"column {column!r} is an integer column: operand {v!r} is not an integer")
        v = int(v)
        if not -(1 << 63) <= v < (1 << 63):
            raise ValueError(f"operand {v} for column {column!r} is out of the int64 range")
        return v & 0xFFFFFFFFFFFFFFFF
    if _is_int(v):
        if abs(int(v)) > (1 << 53):
            raise ValueError(f"column {column!r} is a float column: integer operand {int(v)} beyond 2^53 is not exact in a double")
        v = float(int(v))
    if not _is_float(v):
        raise ValueError(f"column {column!r} is a float column: operand {v!r} is not a number")
    v = float(v)
    if member and v != v:
        raise ValueError(f"isin() on column {column!r}: NaN equals nothing")
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def compile(predicate, dtypes):
    """-> Compiled.  dtypes: {column name: PQV_COL_*} for every column the predicate names (KeyError otherwise).
    A bool operand is 0 / 1 on an integer column (bool Parquet columns are resident as I32) and refused on a float column.
    ValueError: an operand that does not convert exactly to the column's comparison type (a non-integer or beyond-int64 operand
    on an integer column -- an operand beyond int32 on an I32 column is legal, it just never equals anything --, an integer
    beyond +-2^53 on a float column, NaN in isin), more than 32 distinct leaves, a program beyond 63 bytes or 32 stack entries."""
    if not isinstance(predicate, Predicate):
        raise TypeError(f"compile() needs a predicate, got {type(predicate).__name__}")
    leaves, ops, operands, index = [], [], [], {}
    program = bytearray()

    def leaf_index(leaf, neg):
        if leaf.op == _ffi.PQV_OP_MASK:
            key = ("mask", id(leaf.mask), neg)
            a = b = 0
            what = leaf.mask
        else:
            if leaf.column not in dtypes:
                raise KeyError(f"no column named {leaf.column!r}")
            dtype = dtypes[leaf.column]
            if dtype not in _INT_TYPES + _FLOAT_TYPES:
                raise ValueError(f"unknown column type {dtype!r} for column {leaf.column!r}")
            a = b = 0
            if leaf.op != _ffi.PQV_OP_IS_NULL:
                a = _operand_bits(leaf.lo, dtype, leaf.column, leaf.member)
            if leaf.op == _ffi.PQV_OP_BETWEEN:
                b = _operand_bits(leaf.hi, dtype, leaf.column, False)
            key = (leaf.column, leaf.op, a, b, neg)
            what = leaf.column
        i = index.get(key)
        if i is None:
            if len(leaves) == MAX_LEAVES:
                raise ValueError(f"the predicate has more than {MAX_LEAVES} leaves")
            i = index[key] = len(leaves)
            leaves.append(what)
            ops.append(leaf.op | (_ffi.PQV_OP_NOT if neg else 0))
            operands.extend((a, b))
        return i

    def emit(p, neg):
        if isinstance(p, _Not):
            emit(p.inner, not neg)
        elif isinstance(p, _Leaf):
            program.append(leaf_index(p, neg))
        else:
            emit(p.left, neg)
            emit(p.right, neg)
            kind = p.kind
            if neg:         # De Morgan: ~(a & b) = ~a | ~b
                kind = _ffi.PQV_PRED_OR if kind == _ffi.PQV_PRED_AND else _ffi.PQV_PRED_AND
            program.append(kind)

    emit(predicate, False)
    if len(program) > MAX_PROGRAM:
        raise ValueError(f"the predicate's program has {len(program)} bytes, at most {MAX_PROGRAM}")
    depth = deepest = 0
    for c in program:
        depth += -1 if c >= 0x80 else 1
        deepest = max(deepest, depth)
    if deepest > MAX_DEPTH:
        raise ValueError(f"the predicate needs a stack of {deepest}, at most {MAX_DEPTH}")
    return Compiled(leaves, np.array(ops, dtype=np.uint32), np.array(operands, dtype=np.uint64), bytes(program))
