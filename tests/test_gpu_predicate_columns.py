"""Predicate masks on the GPU, continued: to_bytes of a byte-made mask reads the device row image (mask_pack_kernel's output),
a bool operand on a column made from bools, and who closes an attached column."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _searcher(pqv, n, seed):
    rng = np.random.default_rng(seed)
    corpus = pqv.Corpus.upload(rng.random((n, 8), dtype=np.float32))
    rows = rng.permutation(n).astype(np.uint32)
    lists = [np.sort(part) for part in np.array_split(rows, 4)]
    return pqv.Searcher(pqv.Index.from_parts(8, rng.random((4, 8), dtype=np.float32), lists), corpus), corpus


@pytest.mark.parametrize("n", [37, 64, 65, 1031])
def test_to_bytes_of_a_byte_made_mask_is_its_row_image(pqv, n):
    s, corpus = _searcher(pqv, n, 3 + n)
    allowed = (np.random.default_rng(n).integers(0, 3, n) * 5).astype(np.uint8)          # 0, 5, 10: nonzero = allowed
    m = s.row_mask(allowed)
    want = (allowed != 0).astype(np.uint8)
    assert (m.to_bytes() == want).all() and m.count == int(want.sum())
    d = s.row_mask(~pqv.allowed(m))                 # the same image through a MASK leaf
    assert (d.to_bytes() == 1 - want).all() and d.count == n - int(want.sum())
    for x in (m, d, s, corpus):
        x.close()


def test_bool_column_and_operand_and_column_ownership(pqv):
    import pyarrow as pa
    from pq_vector_amd import _ffi
    n = 200
    s, corpus = _searcher(pqv, n, 9)
    flag = np.random.default_rng(1).random(n) < 0.4
    null = np.random.default_rng(2).random(n) < 0.1
    made = s.attach_column("flag", pa.array(flag, pa.bool_(), mask=null))               # uploaded by the searcher: its own
    mine = s.attach_column("mine", pqv.Column.upload(np.arange(n, dtype=np.int64)))     # the caller's
    assert made.dtype == _ffi.PQV_COL_I32 and s.columns == {"flag": made, "mine": mine}
    m = s.row_mask((pqv.col("flag") == True) & (pqv.col("mine") >= 0))                   # noqa: E712
    assert (m.to_bytes() == (flag & ~null)).all()
    m.close()
    m = s.row_mask(pqv.col("flag") != True)                                             # noqa: E712
    assert (m.to_bytes() == (~flag & ~null)).all()
    m.close()
    s.close()
    assert made._h is None and mine._h is not None and mine.rows == n and s.columns == {}
    mine.close()
    corpus.close()
