"""pqv_range_search on the GPU against the numpy range oracle (tests/range_oracle.py) over oracle-built indexes: lims, rows,
distance BITS, n_within and n_candidates exactly -- every layout, both metrics, both output scales, boundary radii, ties,
caps, the multi-pass sort of long segments, probes beyond the kernels' 1024-entry lists, batches beyond 65 535 queries,
agreement with pqv_topk, no side effects on the searcher, the Parquet path and the C3 shape."""
import math
import os

import numpy as np
import pytest

from range_oracle import REF4, SEQ, range_batch, range_query

pytestmark = pytest.mark.gpu

_INDEX = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _index(oracle, n, dim, kc, seed):
    key = (n, dim, kc, seed)
    if key not in _INDEX:
        rng = np.random.default_rng(seed)
        data = rng.random((n, dim), dtype=np.float32)
        _INDEX[key] = (data, oracle.build_index(data, n_clusters=kc, workers=4))
    return _INDEX[key]


def _searcher(pqv, data, oidx, layout="ivf"):
    flags = pqv.PQV_LAYOUT_ROW_ORDER if layout == "row" else pqv.PQV_LAYOUT_IVF_ORDERED
    return pqv.Searcher(pqv.Index.from_bytes(oidx.to_bytes()), pqv.Corpus.upload(data), flags)


def _assert_same(got, exp):
    lims, rows, dist, nw, nc = got
    elims, erows, edist, enw, enc = exp
    assert lims.dtype == np.uint64 and rows.dtype == np.uint32 and dist.dtype == np.float32
    assert (nc == enc).all(), "n_candidates"
    assert (nw == enw).all(), "n_within"
    assert (lims == elims).all(), "lims"
    assert (rows == erows).all(), "rows"
    assert (_bits(dist) == _bits(edist)).all(), "distance bits"


def _cand_out(oidx, data, q, nprobe, metric=REF4, sqrt_out=True):
    _, d, _, _ = range_query(oidx.candidate_rows(q, nprobe), data, q, math.inf, metric=metric, sqrt_out=sqrt_out)
    return d


@pytest.mark.parametrize("dim", [1, 3, 30, 64, 128, 768])
@pytest.mark.parametrize("layout", ["ivf", "row"])
def test_range_shape_matrix(pqv, oracle, dim, layout):
    n = 1500 if dim == 768 else 3000
    data, oidx = _index(oracle, n, dim, 12, dim)
    s = _searcher(pqv, data, oidx, layout)
    rng = np.random.default_rng(dim + 1)
    queries = rng.random((6, dim), dtype=np.float32)
    nprobe = 3
    for metric in (REF4, SEQ):
        for sqrt_out in (False, True):
            outs = np.sort(_cand_out(oidx, data, queries[0], nprobe, metric, sqrt_out))
            radius = float(outs[len(outs) // 2])
            got = s.range_search(queries, radius, nprobe, metric=metric, sqrt_out=sqrt_out)
            exp = range_batch(oidx, data, queries, radius, nprobe, metric=metric, sqrt_out=sqrt_out)
            _assert_same(got, exp)
            assert exp[0][-1] > 0


def test_range_radii_boundaries(pqv, oracle):
    data, oidx = _index(oracle, 3000, 30, 12, 30)
    s = _searcher(pqv, data, oidx)
    queries = np.concatenate([data[[5]], np.random.default_rng(9).random((3, 30), dtype=np.float32)])
    outs = np.sort(_cand_out(oidx, data, queries[0], 4))
    assert outs[0] == 0.0                       # the query is a row of the corpus
    for radius in (0.0, float(outs[1]), float(outs[len(outs) // 2]), float(outs[-1]), math.inf, -1.0, -math.inf):
        for sqrt_out in (True, False):
            r = radius if sqrt_out or radius <= 0 or math.isinf(radius) else radius * radius
            _assert_same(s.range_search(queries, r, 4, sqrt_out=sqrt_out), range_batch(oidx, data, queries, r, 4, sqrt_out=sqrt_out))
    lims, rows, _, nw, nc = s.range_search(queries, float(outs[-1]), 4)
    assert nw[0] == nc[0] and 5 in rows[:lims[1]].tolist()       # the largest candidate distance is inside (<=)
    lims, rows, _, nw, _ = s.range_search(queries, -1.0, 4)
    assert lims[-1] == 0 and (nw == 0).all()
    with pytest.raises(pqv.PqvError, match="radius must not be NaN"):
        s.range_search(queries, math.nan, 4)


def test_range_ties_order_by_position(pqv, oracle):
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "ties_2k_x8.npz"))
    data = np.ascontiguousarray(z["data"], dtype=np.float32)
    oidx = oracle.index_from_bytes(z["w1_blob"].tobytes())
    rng = np.random.default_rng(6)
    queries = rng.integers(0, 3, size=(40, data.shape[1])).astype(np.float32)
    for layout in ("ivf", "row"):
        s = _searcher(pqv, data, oidx, layout)
        for radius in (1.0, 2.0, math.sqrt(3.0)):
            for mr in (0, 7):
                got = s.range_search(queries, radius, 3, max_results=mr)
                _assert_same(got, range_batch(oidx, data, queries, radius, 3, max_results=mr))


def test_range_caps(pqv, oracle):
    data, oidx = _index(oracle, 3000, 64, 12, 64)
    s = _searcher(pqv, data, oidx)
    queries = np.random.default_rng(11).random((8, 64), dtype=np.float32)
    lens = np.diff(oidx.list_off.astype(np.int64))
    cap = int(lens.max() + lens.min() // 2)               # inside the second probed list for most queries
    outs = np.sort(_cand_out(oidx, data, queries[0], 4))
    radius = float(outs[len(outs) // 3])
    full = s.range_search(queries, radius, 4)
    _assert_same(full, range_batch(oidx, data, queries, radius, 4))
    _assert_same(s.range_search(queries, radius, 4, max_candidates=cap), range_batch(oidx, data, queries, radius, 4, max_candidates=cap))
    for mr in (1, 5, 50):
        got = s.range_search(queries, radius, 4, max_results=mr)
        _assert_same(got, range_batch(oidx, data, queries, radius, 4, max_results=mr))
        assert (got[3] == full[3]).all()                  # n_within is the full count
        for q in range(len(queries)):
            a, b = full[0][q], full[0][q + 1]
            k = got[0][q + 1] - got[0][q]
            assert k == min(mr, b - a)
            assert (got[1][got[0][q]:got[0][q + 1]] == full[1][a:a + k]).all()


def test_range_long_segments_multi_pass_sort(pqv, oracle):
    rng = np.random.default_rng(21)
    n, dim = 262144, 4
    data = rng.random((n, dim), dtype=np.float32)
    oidx = oracle.build_index(data, n_clusters=16, workers=8, max_iters=3)
    s = _searcher(pqv, data, oidx)
    q1 = np.full((1, dim), 0.5, np.float32)
    got = s.range_search(q1, math.inf, 16)
    assert got[3][0] == n > 200_000
    _assert_same(got, range_batch(oidx, data, q1, math.inf, 16))
    # a batch mixing empty, small, mid-size and huge segments; then a cap inside the long ones
    queries = np.array([[0.5] * 4, [0.0] * 4, [100.0] * 4, [0.3, 0.6, 0.5, 0.4], [1.0, 0.0, 1.0, 0.0]], np.float32)
    for radius, mr in ((0.6, 0), (0.08, 0), (0.6, 10000), (0.6, 3)):
        got = s.range_search(queries, radius, 16, max_results=mr)
        exp = range_batch(oidx, data, queries, radius, 16, max_results=mr)
        _assert_same(got, exp)
    nw = s.range_search(queries, 0.6, 16)[3]
    assert nw[2] == 0 and nw[0] > 100_000 and 0 < nw[1] < nw[0]


def test_range_wide_probe(pqv, oracle):
    rng = np.random.default_rng(31)
    n, dim, kc = 15000, 8, 1500
    data = rng.random((n, dim), dtype=np.float32)
    cent = rng.random((kc, dim), dtype=np.float32)
    assign = rng.integers(0, kc, size=n)
    lists = [np.nonzero(assign == c)[0].astype(np.uint32).tolist() for c in range(kc)]
    idx = pqv.Index.from_parts(dim, cent.reshape(-1).tolist(), lists)
    oidx = oracle.index_from_bytes(idx.to_bytes())
    s = pqv.Searcher(idx, pqv.Corpus.upload(data))
    queries = rng.random((5, dim), dtype=np.float32)
    for nprobe in (1100, 1500, 4000):
        for radius, mc in ((0.5, 0), (math.inf, 0), (0.6, 5000)):
            got = s.range_search(queries, radius, nprobe, max_candidates=mc)
            _assert_same(got, range_batch(oidx, data, queries, radius, nprobe, max_candidates=mc))


def test_range_big_batch(pqv, oracle):
    data, oidx = _index(oracle, 5000, 4, 8, 4)
    s = _searcher(pqv, data, oidx)
    rng = np.random.default_rng(41)
    nq = 66000
    queries = rng.random((nq, 4), dtype=np.float32)
    radius = 0.08
    lims, rows, dist, nw, nc = s.range_search(queries, radius, 2)
    assert len(lims) == nq + 1 and lims[-1] > 0
    off = 0
    for c0 in range(0, nq, 1000):
        cl, cr, cd, cw, cn = s.range_search(queries[c0:c0 + 1000], radius, 2)
        assert (lims[c0:c0 + len(cl)] - lims[c0] == cl).all()
        assert (rows[off:off + cl[-1]] == cr).all() and (_bits(dist[off:off + cl[-1]]) == _bits(cd)).all()
        assert (nw[c0:c0 + 1000] == cw).all() and (nc[c0:c0 + 1000] == cn).all()
        off += int(cl[-1])
    assert off == lims[-1]
    for q in rng.choice(nq, 50, replace=False):
        r, d, w, c = range_query(oidx.candidate_rows(queries[q], 2), data, queries[q], radius)
        a, b = lims[q], lims[q + 1]
        assert (rows[a:b] == r).all() and (_bits(dist[a:b]) == _bits(d)).all() and nw[q] == w and nc[q] == c


def test_range_agrees_with_topk(pqv, oracle):
    data, oidx = _index(oracle, 3000, 30, 12, 30)
    s = _searcher(pqv, data, oidx)
    queries = np.random.default_rng(51).random((40, 30), dtype=np.float32)
    rows, dist, nf, _ = s.topk(queries, 11, 4)
    checked = 0
    for q in range(len(queries)):
        d = dist[q]
        if nf[q] < 11 or len(np.unique(d[:11])) < 11:
            continue
        lims, r, rd, _, _ = s.range_search(queries[q:q + 1], float(d[9]), 4, max_results=10)
        assert lims[-1] == 10
        assert (r == rows[q, :10]).all() and (_bits(rd) == _bits(d[:10])).all()
        checked += 1
    assert checked >= 30


def test_range_leaves_topk_and_counters_as_topk(pqv, oracle):
    data, oidx = _index(oracle, 3000, 64, 12, 64)
    queries = np.random.default_rng(61).random((20, 64), dtype=np.float32)
    s = _searcher(pqv, data, oidx)
    before = s.topk(queries, 10, 4)
    c0 = s.counters()
    s.range_search(queries, 1.5, 4, max_candidates=700)
    s.range_search(queries[:3], math.inf, 12)
    c1 = s.counters()
    after = s.topk(queries, 10, 4)
    for a, b in zip(before, after):
        assert (np.asarray(a).view(np.uint8) == np.asarray(b).view(np.uint8)).all()
    # counters: as topk calls of the same shapes on a fresh searcher
    t = _searcher(pqv, data, oidx)
    t0 = t.counters()
    t.topk(queries, 10, 4, max_candidates=700)
    t.topk(queries[:3], 10, 12)
    t1 = t.counters()
    for key in ("queries", "candidate_rows", "embeddings_fetched"):
        assert c1[key] - c0[key] == t1[key] - t0[key], key


def test_range_builder_parquet_path(pqv, oracle, tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    rng = np.random.default_rng(71)
    n, dim = 600, 6
    vecs = rng.random((n, dim), dtype=np.float32)
    t = pa.table({"id": pa.array(np.arange(n, dtype=np.int64)),
                  "vec": pa.array(vecs.tolist(), type=pa.list_(pa.float32()))})
    src, out = str(tmp_path / "s.parquet"), str(tmp_path / "o.parquet")
    pq.write_table(t, src, row_group_size=128)
    pqv.IndexBuilder(src, "vec").n_clusters(8).build_new(out)
    idx, _ = pqv.read_index_from_parquet(out)
    oidx = oracle.index_from_bytes(idx.to_bytes())
    q = rng.random(dim, dtype=np.float32)
    for radius, mr in ((0.5, 0), (0.7, 5), (math.inf, 0)):
        b = pqv.RangeBuilder(out, q).radius(radius).nprobe(3)
        if mr:
            b = b.max_results(mr)
        res = b.search()
        er, ed, _, _ = range_query(oidx.candidate_rows(q, 3), vecs, q, radius, max_results=mr)
        assert [r.row_idx for r in res] == er.tolist()
        assert _bits([r.distance for r in res]).tolist() == _bits(ed).tolist()


def test_range_full_size_c3(pqv, oracle):
    import torch
    import bench
    n, dim, kc, nprobe, _ = bench.WORKLOADS["c3"]
    dev = torch.device("cuda", 0)
    corpus_t = bench.synth(torch, dev, 1234, n, dim)
    q_t = bench.synth(torch, dev, 7, 16, dim)
    torch.cuda.synchronize()
    corpus = pqv.Corpus.from_device_ptr(corpus_t.data_ptr(), n, dim, device=0, keepalive=corpus_t)
    index = pqv.IndexBuilder(corpus).n_clusters(kc).max_iters(20).seed(42).workers(os.cpu_count() or 1).build()
    s = pqv.Searcher(index, corpus)
    oidx = oracle.index_from_bytes(index.to_bytes())
    queries = q_t.cpu().numpy()
    _, d100, _, _ = s.topk(queries[:1], 100, nprobe)
    radius = float(d100[0, 99])
    lims, rows, dist, nw, nc = s.range_search(queries, radius, nprobe)
    assert 20 < lims[-1] / 16 < 2000
    for q in range(16):
        cand = oidx.candidate_rows(queries[q], nprobe)
        r, d, w, c = range_query(cand, lambda ids: corpus.fetch_rows(ids), queries[q], radius)
        a, b = lims[q], lims[q + 1]
        assert nc[q] == c and nw[q] == w
        assert (rows[a:b] == r).all() and (_bits(dist[a:b]) == _bits(d)).all()
