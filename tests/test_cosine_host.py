"""PQV_COSINE without a GPU: the float32 restatement of sq / r / n (tests/cosine_ref.py) against the C oracle's chain and its
own invariants, and the argument checks of the builders' metric()."""
import numpy as np
import pytest

from cosine_ref import half, normalise, r, sq


def test_sq_is_the_oracle_chain_against_zero(oracle):
    rng = np.random.default_rng(5)
    for dim in (1, 3, 4, 8, 30, 128, 769):
        x = (rng.standard_normal((7, dim)) * 3).astype(np.float32)
        s = sq(x)
        zero = np.zeros(dim, dtype=np.float32)
        for i in range(len(x)):
            assert np.float32(s[i]).view(np.uint32) == np.float32(oracle.l2_ref4(x[i], zero)).view(np.uint32)


def test_r_and_n_are_float32_operations():
    rng = np.random.default_rng(6)
    x = rng.random((50, 30), dtype=np.float32) - np.float32(0.5)
    s = sq(x)
    rr = r(x)
    assert rr.dtype == np.float32
    for i in range(len(x)):
        assert rr[i] == np.float32(1.0) / np.sqrt(np.float32(s[i]))
        assert (normalise(x)[i] == x[i] * rr[i]).all()
    # unit length up to rounding
    assert np.allclose(sq(normalise(x)), 1.0, rtol=1e-5)


def test_zero_rows_normalise_to_zero():
    x = np.zeros((3, 8), dtype=np.float32)
    x[1, 2] = 1e-30                                   # its square underflows: sq == 0, r == 0
    x[2, 0] = 2.0
    n = normalise(x)
    assert (r(x)[:2] == 0).all() and (n[:2] == 0).all()
    assert n[2, 0] == 1.0 and (n[2, 1:] == 0).all()


def test_power_of_two_scaling_gives_the_same_bits():
    rng = np.random.default_rng(7)
    x = rng.random((20, 3 * 128 + 3), dtype=np.float32)
    for scale in (2.0, 0.25, 1024.0):
        assert (normalise(x * np.float32(scale)).view(np.uint32) == normalise(x).view(np.uint32)).all()


def test_half_is_exact():
    d2 = np.array([0.0, 1.0, 3.999, 1e-20, np.inf], dtype=np.float32)
    assert (half(d2) * np.float32(2) == d2).all()


@pytest.mark.parametrize("builder", ["TopkBuilder", "RangeBuilder", "TableTopkBuilder", "TableRangeBuilder"])
def test_builder_metric_arguments(builder):
    import pq_vector_amd as pqv
    cls = getattr(pqv, builder)
    src = ["a.parquet", "b.parquet"] if builder.startswith("Table") else "a.parquet"
    b = cls(src, np.zeros(4, dtype=np.float32))
    assert b._metric == pqv.PQV_L2SQ_REF4                                    # the default is unchanged
    assert b.metric(pqv.PQV_COSINE) is b and b._metric == pqv.PQV_COSINE
    assert b.metric(pqv.PQV_L2SQ_REF4) is b and b._metric == pqv.PQV_L2SQ_REF4
    for bad in (pqv.PQV_L2SQ_SEQ, pqv.PQV_L2SQ_MFMA, 7, -1, "cosine", None, True, 2.0):
        with pytest.raises(pqv.PqvError) as e:
            b.metric(bad)
        assert e.value.code == pqv._ffi.PQV_ERR_INVALID and "unknown metric" in str(e.value)
    assert b._metric == pqv.PQV_L2SQ_REF4                                    # a refused value changes nothing


def test_prepare_flag_is_exported():
    import pq_vector_amd as pqv
    assert pqv.PQV_PREPARE_COSINE == 0x10 and "PQV_PREPARE_COSINE" in pqv.__all__
    flags = (pqv.PQV_LAYOUT_ROW_ORDER, pqv.PQV_RELEASE_ROW_ORDER, pqv.PQV_RELEASE_IF_COPIED, pqv.PQV_TABLE_CAP_ROUND_ROBIN)
    assert all(pqv.PQV_PREPARE_COSINE & f == 0 for f in flags)
