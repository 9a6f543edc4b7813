"""One case of tests/mutated_cases.py relocated onto "far" rows of a corpus as large as the workload's (test infrastructure: nothing
here calls the library under test).

An index does not have to cover its corpus: the dense case's n2 rows are placed, through a strictly increasing map R, around the four
rows of a big row matrix at which 32-bit address arithmetic breaks -- the rows that straddle 2^31 and 2^32 BYTES and 2^31 and 2^32
ELEMENTS -- and every other row of the big corpus is filler that no list holds.  With T(x) = x // dim:

    dense rows                    rows of the big corpus
    [0, 768)                      [0, 768)
    [768, 1536)                   768 consecutive rows centred on T(2^31 / 4)          (2^31 bytes)
    [1536, 2304)                  768 consecutive rows centred on T(2^32 / 4)          (2^32 bytes)
    [2304, 3072)                  768 consecutive rows centred on T(2^31)              (2^31 elements)
    [3072, 4096)  first append    1024 consecutive rows centred on T(2^32)             (2^32 elements)
    [4096, 4608)  second append   512 consecutive rows, starting 1000 rows behind the run before

The two appended ranges are contiguous, so Index.append(corpus, first_row=R[n0], n_rows=n1 - n0) indexes exactly those rows.  R is
monotone: every order that looks at row ids or list positions -- the reference's heap included -- is the dense case's, so the answer
of every call on the far index is mutated_cases.expect() on the dense model with its `rows` mapped through R (relocate).

FarModel is one state as tests/mode_calls.py's Handles reads it: masks and columns of n_far entries, the dense arrays scattered
through R.  A filler row gets what makes a wrong fetch change an answer instead of vanishing: its mask bits set, query 0's tenant, a
valid ts inside query 0's range, doc 0."""
import numpy as np

import mutated_cases as mc

RUN = 768                 # rows per run of the built index
GAP = 1000                # filler rows between the two appended runs


def break_rows(dim):
    """the rows whose first element lies below and whose last element lies above 2^31 bytes, 2^32 bytes, 2^31 elements and 2^32
    elements of an f32 row matrix"""
    rows = [(1 << 31) // (4 * dim), (1 << 32) // (4 * dim), (1 << 31) // dim, (1 << 32) // dim]
    for r, x in zip(rows, (1 << 29, 1 << 30, 1 << 31, 1 << 32)):          # (in elements)
        assert r * dim < x < (r + 1) * dim - 1
    return rows


def row_map(dim, n0, n1, n2):
    """-> (R int64 [n2], n_far): dense row id -> row id of the big corpus"""
    assert n0 == 4 * RUN and n1 > n0 and n2 > n1
    b = break_rows(dim)
    R = np.empty(n2, np.int64)
    R[:RUN] = np.arange(RUN)
    for i in range(3):
        R[(i + 1) * RUN:(i + 2) * RUN] = b[i] - RUN // 2 + np.arange(RUN)
    R[n0:n1] = b[3] - (n1 - n0) // 2 + np.arange(n1 - n0)
    R[n1:] = R[n1 - 1] + 1 + GAP + np.arange(n2 - n1)
    return R, int(R[-1]) + 1


class FarCase:
    """The relocation of one shape of mutated_cases.SHAPES"""

    def __init__(self, oracle, name):
        self.name = name
        self.case = c = mc.case(oracle, name)
        self.dim = c.dim
        self.breaks = break_rows(c.dim)
        self.R, self.n_far = row_map(c.dim, c.n0, c.n1, c.n2)
        self._models = {}

    def rows(self, ids):
        """dense row ids -> far row ids (uint32), mutated_cases.EMPTY and ids past the dense corpus kept as they are"""
        ids = np.asarray(ids)
        inside = ids.astype(np.int64) < len(self.R)
        return np.where(inside, self.R[np.where(inside, ids, 0).astype(np.int64)], ids.astype(np.int64)).astype(np.uint32)

    def lists(self, lists):
        return [self.R[np.asarray(l, np.int64)].astype(np.uint32) for l in lists]

    def bound(self, dense_bound):
        """the far row bound of an index whose dense bound is n0, n1 or n2 (the row before it is, or was, indexed)"""
        return int(self.R[dense_bound - 1]) + 1 if dense_bound else 0

    def scatter(self, dense, filler, dtype=None):
        out = np.full(self.n_far, filler, dtype or np.asarray(dense).dtype)
        out[self.R] = dense
        return out

    def read(self, first_element, fill):
        """the dim floats a read at element offset `first_element` of the big matrix returns (filler rows hold `fill`): what a
        kernel with a wrapped offset would compute on"""
        e = int(first_element) + np.arange(self.dim, dtype=np.int64)
        row, col = e // self.dim, e % self.dim
        assert row[0] >= 0 and row[-1] < self.n_far
        at = np.searchsorted(self.R, row)
        real = (at < len(self.R)) & (self.R[np.minimum(at, len(self.R) - 1)] == row)
        out = np.full(self.dim, fill, np.float32)
        out[real] = self.case.X[at[real], col[real]]
        return out

    def model(self, state):
        if state not in self._models:
            self._models[state] = FarModel(self, self.case.models[state])
        return self._models[state]

    def relocate(self, expected):
        """an expect() result on the dense model -> the result on the far index: `rows` through R, everything else as it is"""
        out = dict(expected)
        out["rows"] = self.rows(expected["rows"])
        return out


class FarModel:
    """One state over the big corpus: what mode_calls.Handles reads (n, masks, cols, case), and the lists"""

    def __init__(self, far, dense):
        assert dense.n == len(far.R), "the compacted state has a corpus of its own"
        c = dense.case
        self.far, self.dense, self.case, self.name = far, dense, c, dense.name
        self.n, self.dim, self.C = far.n_far, dense.dim, dense.C
        self.lists = far.lists(dense.lists)
        self.bound = far.bound(dense.bound)
        key0 = int(c.qkeys[0])
        lo, hi = c.filters["range"][2]
        ts0 = int(lo[0]) + 500
        assert int(lo[0]) <= ts0 <= int(hi[0]) and c.filters["eq"][2][0] == key0
        filler = {"tenant": key0, "ts": ts0, "doc": 0}
        self.masks = {n: far.scatter(a, True) for n, a in dense.masks.items()}
        self.cols = {n: (far.scatter(v, filler[n]), None if ok is None else far.scatter(ok, True)) for n, (v, ok) in dense.cols.items()}

    def in_lists(self):
        a = np.zeros(self.n, bool)
        for l in self.lists:
            a[np.asarray(l, np.int64)] = True
        return a


_MADE = {}


def far_case(oracle, name):
    if name not in _MADE:
        _MADE[name] = FarCase(oracle, name)
    return _MADE[name]
