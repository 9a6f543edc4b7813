"""PQV_DOT without a GPU: the constant and the builders' metric(), and the numpy model of tests/dot_ref.py against the C oracle's
chain, the recursive-summation error bound and its own invariants."""
import os

import numpy as np
import pytest

import dot_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_constant_is_exported_and_in_the_header():
    import pq_vector_amd as pqv
    assert pqv.PQV_DOT == 4 and pqv._ffi.PQV_DOT == 4 and "PQV_DOT" in pqv.__all__
    assert pqv.PQV_DOT not in (pqv.PQV_L2SQ_REF4, pqv.PQV_L2SQ_SEQ, pqv.PQV_COSINE, pqv.PQV_L2SQ_MFMA)
    header = open(os.path.join(ROOT, "include", "pqv.h")).read()
    assert "#define PQV_DOT         4" in header
    assert "PQV_DOT takes k <= 1024 and at most 1024 probed lists" in " ".join(header.replace(" *", " ").split())
    assert "pub const PQV_DOT: c_int = 4;" in open(os.path.join(ROOT, "bindings", "rust", "src", "sys.rs")).read()


@pytest.mark.parametrize("builder", ["TopkBuilder", "RangeBuilder", "TableTopkBuilder", "TableRangeBuilder"])
def test_builder_metric_accepts_dot_and_refuses_what_it_refused(builder):
    import pq_vector_amd as pqv
    cls = getattr(pqv, builder)
    src = ["a.parquet", "b.parquet"] if builder.startswith("Table") else "a.parquet"
    b = cls(src, np.zeros(4, dtype=np.float32))
    assert b._metric == pqv.PQV_L2SQ_REF4
    assert b.metric(pqv.PQV_DOT) is b and b._metric == pqv.PQV_DOT
    for bad in (pqv.PQV_L2SQ_SEQ, pqv.PQV_L2SQ_MFMA, 7, -1, "dot", "4", None, True, False, 4.0):
        with pytest.raises(pqv.PqvError) as e:
            b.metric(bad)
        assert e.value.code == pqv._ffi.PQV_ERR_INVALID and "unknown metric" in str(e.value)
    assert b._metric == pqv.PQV_DOT                                          # a refused value changes nothing
    assert b.metric(pqv.PQV_COSINE) is b and b.metric(pqv.PQV_L2SQ_REF4) is b and b._metric == pqv.PQV_L2SQ_REF4


@pytest.mark.parametrize("dim", [1, 3, 4, 8, 30, 128, 769])
def test_chain_of_x_with_itself_is_the_oracle_chain_against_zero(oracle, dim):
    rng = np.random.default_rng(100 + dim)
    x = (rng.standard_normal((9, dim)) * 3).astype(np.float32)
    s = dot_ref.dot_chain(x, x)
    assert s.dtype == np.float32
    zero = np.zeros(dim, dtype=np.float32)
    for i in range(len(x)):
        assert _bits(s[i:i + 1])[0] == _bits(np.float32(oracle.l2_ref4(x[i], zero)))[()]
        assert _bits(dot_ref.dot_chain(x[i], x[i:i + 1]))[0] == _bits(s[i:i + 1])[0]      # one query against rows == row by row


@pytest.mark.parametrize("dim", [1, 3, 4, 8, 30, 128, 769])
def test_dist_is_within_the_recursive_summation_bound(dim):
    """dim rounded products and fewer than dim rounded adds: |fl - exact| <= gamma_dim * sum |q_i x_i| with gamma_dim <=
    1.01 * dim * 2^-24 for these dims (Higham, Accuracy and Stability, 3.1)."""
    rng = np.random.default_rng(200 + dim)
    x = rng.standard_normal((200, dim)).astype(np.float32)
    q = rng.standard_normal(dim).astype(np.float32)
    d = dot_ref.dist(q, x)
    exact = (x.astype(np.float64) * q.astype(np.float64)).sum(axis=1)
    mag = (np.abs(x.astype(np.float64)) * np.abs(q.astype(np.float64))).sum(axis=1)
    assert (np.abs(d.astype(np.float64) + exact) <= 1.01 * dim * 2.0 ** -24 * mag).all()


def test_no_negative_zero():
    rng = np.random.default_rng(3)
    cases = []
    for dim in (1, 3, 4, 8, 30):
        x = rng.integers(-3, 4, (500, dim)).astype(np.float32)
        x[::7] = 0.0
        x[1::7] = -0.0
        for q in (np.zeros(dim, np.float32), -np.zeros(dim, np.float32), rng.integers(-3, 4, dim).astype(np.float32)):
            cases.append(dot_ref.dist(q, x))
    # products that underflow to signed zeros
    tiny = np.full((4, 8), 1e-30, dtype=np.float32)
    tiny[1] *= -1
    cases.append(dot_ref.dist(np.full(8, 1e-30, np.float32), tiny))
    cases.append(dot_ref.dist(np.full(8, -1e-30, np.float32), tiny))
    d = np.concatenate(cases)
    zeros = d == 0
    assert zeros.sum() > 100
    assert (_bits(d[zeros]) == 0).all()


def test_ord_bits_is_strictly_monotone():
    den = np.array([1, 2, 0x7FFFFF], dtype=np.uint32).view(np.float32)       # denormals
    rng = np.random.default_rng(4)
    vals = np.concatenate([[-np.inf, np.inf, 0.0, 1e-38, -1e-38, 3.4e38, -3.4e38, 1.0, -1.0], den, -den,
                           rng.standard_normal(500) * 100, rng.standard_normal(500) * 1e-3]).astype(np.float32)
    vals = np.unique(vals)                                                   # sorted, distinct as VALUES (+0.0 == -0.0: one of them)
    o = dot_ref.ord_bits(vals).astype(np.int64)
    assert (np.diff(o) > 0).all()
    # -0.0 sorts directly below +0.0, both between the denormals of either sign
    z = dot_ref.ord_bits(np.array([-den[0], -0.0, 0.0, den[0]], dtype=np.float32)).astype(np.int64)
    assert (np.diff(z) == 1).all()
    # mixed signs sort like their values
    mixed = rng.standard_normal(1000).astype(np.float32)
    assert (mixed[np.argsort(dot_ref.ord_bits(mixed), kind="stable")] == np.sort(mixed)).all()


def test_model_topk_breaks_exact_ties_by_position():
    rng = np.random.default_rng(5)
    n, dim, kc = 4000, 8, 6
    data = rng.integers(-3, 4, (n, dim)).astype(np.float32)
    cent = rng.integers(-3, 4, (kc, dim)).astype(np.float32)
    assign = rng.integers(0, kc, n)
    lists = [np.nonzero(assign == c)[0].astype(np.uint32) for c in range(kc)]
    q = rng.integers(-3, 4, dim).astype(np.float32)
    k = 50
    rows, d, nf, nc = dot_ref.topk_ref(q, cent, lists, data, k, 3)
    cand = dot_ref.candidates(q, cent, lists, 3)
    assert nf == k and nc == len(cand) == sum(len(lists[c]) for c in dot_ref.probe(q, cent, 3))
    assert len(np.unique(d)) < k / 2                                         # many exact ties
    pos_of = {int(r): i for i, r in enumerate(cand)}
    pos = np.array([pos_of[int(r)] for r in rows])
    for i in range(k - 1):
        assert d[i] < d[i + 1] or (d[i] == d[i + 1] and pos[i] < pos[i + 1])
    # exact on integers: the f64 dot products, and the k smallest of them
    exact = -(data[cand.astype(np.int64)].astype(np.float64) @ q.astype(np.float64))
    assert (d == exact[pos]).all() and d[-1] <= np.sort(exact)[k - 1]
    # a cap before an allow array, positions unmasked
    allow = rng.random(n) < 0.5
    rows2, d2, nf2, nc2 = dot_ref.topk_ref(q, cent, lists, data, k, 3, max_candidates=700, allow=allow)
    assert nc2 == nc and all(allow[int(r)] and pos_of[int(r)] < 700 for r in rows2[:nf2])
    rr, rd, nw, _ = dot_ref.range_ref(q, cent, lists, data, float(d[10]), 3, max_results=5)
    assert nw == int((exact <= d[10]).sum()) and (rr == rows[:5]).all() and (_bits(rd) == _bits(d[:5])).all()
