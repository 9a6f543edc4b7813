"""Table searchers on the GPU (pqv_table_searcher_create): a one-file table is an ordinary searcher; a table of F files gives
what F per-file searchers merged with pqv_merge_topk give, and the distances of the numpy chains over the concatenation of the
oracle's per-file candidate_rows (file 0's, then file 1's, ... with rows shifted by row_base)."""
import math

import numpy as np
import pytest

from range_oracle import REF4, l2_chain, range_query

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Table:
    """F files of unequal sizes / cluster counts, each indexed on its own by the oracle, and one corpus holding all of
    them (`gap` filler rows between the files: the row ranges need not touch)."""

    def __init__(self, pqv, oracle, rng, sizes, kcs, dim, gap=3, integer=False, flags=None):
        self.files, self.oidx, self.idx, self.row_base = [], [], [], []
        parts, at = [], 0
        for n, kc in zip(sizes, kcs):
            data = (rng.integers(0, 3, (n, dim)).astype(np.float32) if integer else rng.random((n, dim), dtype=np.float32))
            o = oracle.build_index(data, n_clusters=kc, max_iters=5, workers=1)
            self.files.append(data)
            self.oidx.append(o)
            self.idx.append(pqv.Index.from_bytes(o.to_bytes()))
            parts.append(rng.random((gap, dim), dtype=np.float32))
            at += gap
            self.row_base.append(at)
            parts.append(data)
            at += n
        self.data = np.ascontiguousarray(np.concatenate(parts))
        self.corpus = pqv.Corpus.upload(self.data)
        kw = {} if flags is None else {"flags": flags}
        self.s = pqv.TableSearcher(self.idx, self.corpus, self.row_base, **kw)
        self.kcs = [o.n_clusters for o in self.oidx]

    def cand(self, q, nprobe):
        return np.concatenate([o.candidate_rows(q, nprobe).astype(np.int64) + b for o, b in zip(self.oidx, self.row_base)]).astype(np.uint32)

    def probe(self, q, nprobe):
        cb = np.concatenate([[0], np.cumsum(self.kcs)])
        return np.concatenate([np.asarray(o.find_closest_centroids(q, nprobe), dtype=np.int64) + cb[f]
                               for f, o in enumerate(self.oidx)]).astype(np.uint32)

    def expect_topk(self, q, k, nprobe, metric=REF4):
        cand = self.cand(q, nprobe)
        d2 = l2_chain(self.data[cand], q, metric)
        order = np.lexsort((np.arange(len(cand)), d2))[:k]
        return cand[order], d2[order], len(cand)


def _device_topk(torch, s, queries, k, nprobe, **kw):
    dev = torch.device("cuda", 0)
    q_t = torch.from_numpy(np.ascontiguousarray(queries, dtype=np.float32)).to(dev)
    nq = len(queries)
    rows_t = torch.full((nq, k), -1, dtype=torch.int32, device=dev)
    dist_t = torch.full((nq, k), float("inf"), dtype=torch.float32, device=dev)
    nf_t = torch.zeros(nq, dtype=torch.int32, device=dev)
    nc_t = torch.zeros(nq, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    s.topk_device(q_t.data_ptr(), nq, k, nprobe, rows_t.data_ptr(), dist_t.data_ptr(), nf_t.data_ptr(), nc_t.data_ptr(), sqrt_out=False, **kw)
    torch.cuda.synchronize()
    return (rows_t.cpu().numpy().view(np.uint32), dist_t.cpu().numpy(), nf_t.cpu().numpy().astype(np.uint32),
            nc_t.cpu().numpy().astype(np.uint64))


@pytest.mark.parametrize("dim", [8, 30, 128, 768])
def test_one_file_table_is_an_ordinary_searcher(pqv, oracle, dim):
    import torch
    rng = np.random.default_rng(dim)
    n = 6000 if dim < 768 else 3000
    data = rng.random((n, dim), dtype=np.float32)
    o = oracle.build_index(data, n_clusters=24, max_iters=5, workers=1)
    corpus = pqv.Corpus.upload(data)
    plain = pqv.Searcher(pqv.Index.from_bytes(o.to_bytes()), corpus)
    table = pqv.TableSearcher([pqv.Index.from_bytes(o.to_bytes())], corpus, [0])
    queries = rng.random((40, dim), dtype=np.float32)
    for nq in (1, 7, 40):
        for metric in (pqv.PQV_L2SQ_REF4, pqv.PQV_L2SQ_SEQ):
            a = plain.topk(queries[:nq], 10, 3, metric=metric)
            b = table.topk(queries[:nq], 10, 3, metric=metric)
            for x, y in zip(a, b):
                assert (np.asarray(x).view(np.uint32) == np.asarray(y).view(np.uint32)).all()
        a = _device_topk(torch, plain, queries[:nq], 10, 3)
        b = _device_topk(torch, table, queries[:nq], 10, 3)
        for x, y in zip(a, b):
            assert (np.asarray(x).view(np.uint32) == np.asarray(y).view(np.uint32)).all()
        ra = plain.range_search(queries[:nq], 0.9 * math.sqrt(dim / 6), 3)
        rb = table.range_search(queries[:nq], 0.9 * math.sqrt(dim / 6), 3)
        for x, y in zip(ra, rb):
            assert (np.asarray(x).view(np.uint8) == np.asarray(y).view(np.uint8)).all()
    for q in queries[:3]:
        assert (plain.probe(q, 5) == table.probe(q, 5)).all()
        assert (plain.candidate_rows(q, 5) == table.candidate_rows(q, 5)).all()
    ca, cb = plain.counters(), table.counters()
    for key in ("queries", "candidate_rows", "embeddings_fetched"):
        assert ca[key] == cb[key], key
    assert table.split_rows(np.array([0, n - 1], np.uint32))[0].tolist() == [0, 0]
    assert "table" not in plain.describe(1024, 10, 3)
    assert "table of 1 files" in table.describe(1024, 10, 3)


@pytest.mark.parametrize("F", [2, 5, 17])
def test_table_topk_device_equals_per_file_search_merged(pqv, oracle, F):
    import torch
    rng = np.random.default_rng(100 + F)
    dim = 32
    sizes = [int(x) for x in rng.integers(80, 900, F)]
    kcs = [2] + [int(x) for x in rng.integers(1, 12, F - 1)]
    t = Table(pqv, oracle, rng, sizes, kcs, dim)
    per_file = [pqv.Searcher(ix, pqv.Corpus.upload(d)) for ix, d in zip(t.idx, t.files)]
    nprobe = 4                              # (some files have fewer clusters)
    assert any(kc < nprobe for kc in t.kcs)
    queries = rng.random((1024, dim), dtype=np.float32)
    for nq in (1, 7, 1024):
        for k in (1, 10, 100):
            rows, dist, nf, nc = _device_topk(torch, t.s, queries[:nq], k, nprobe)
            pr, pd, pn = [], [], []
            for s_f, b in zip(per_file, t.row_base):
                r, d, n_f, _ = _device_topk(torch, s_f, queries[:nq], k, nprobe)
                r = np.where(r == 0xFFFFFFFF, r, r.astype(np.int64) + b).astype(np.uint32)
                pr.append(r); pd.append(d); pn.append(n_f)
            md, mr, _, mc = pqv.merge_topk(np.stack(pd), np.stack(pr), np.stack(pn))
            assert (nf == mc).all()
            for q in range(nq):
                m = int(nf[q])
                assert (rows[q, :m] == mr[q, :m]).all()
                assert (_bits(dist[q, :m]) == _bits(md[q, :m])).all()
            for q in (range(nq) if nq < 1024 else range(0, 1024, 97)):
                er, ed, ncand = t.expect_topk(queries[q], k, nprobe)
                assert nc[q] == ncand
                assert (rows[q, :len(er)] == er).all() and (_bits(dist[q, :len(er)]) == _bits(ed)).all()
    for q in queries[:4]:
        assert (t.s.probe(q, nprobe) == t.probe(q, nprobe)).all()
        assert (t.s.candidate_rows(q, nprobe) == t.cand(q, nprobe)).all()


def test_table_topk_seq_ties_equal_the_reference_heap(pqv, oracle):
    rng = np.random.default_rng(5)
    t = Table(pqv, oracle, rng, [300, 120, 500, 60], [6, 3, 9, 2], 12, integer=True)
    queries = rng.integers(0, 3, (24, 12)).astype(np.float32)
    for k in (1, 10, 100):
        rows, d2, nf, nc = t.s.topk(queries, k, 2, metric=pqv.PQV_L2SQ_SEQ, sqrt_out=False)
        for q in range(len(queries)):
            cand = t.cand(queries[q], 2)
            assert nc[q] == len(cand)
            orow, od2 = oracle.topk_df(t.data, cand, queries[q], k)          # VectorTopKExec's one heap over the files
            m = len(orow)
            assert nf[q] == m
            assert (rows[q, :m] == orow).all() and (_bits(d2[q, :m]) == _bits(od2)).all()
    assert t.s.counters()["exact_replays"] > 0             # the case does hold ties


def test_table_range_search_equals_the_restatement(pqv, oracle):
    rng = np.random.default_rng(9)
    t = Table(pqv, oracle, rng, [4000, 700, 2500], [4, 7, 2], 16)
    queries = rng.random((9, 16), dtype=np.float32)
    for radius in (0.9, 1.3, math.inf):            # inf: one file's segment is thousands long (the merge-path sort)
        lims, rows, dist, nw, nc = t.s.range_search(queries, radius, 3)
        for q in range(len(queries)):
            r, d, w, c = range_query(t.cand(queries[q], 3), t.data, queries[q], radius)
            a, b = lims[q], lims[q + 1]
            assert nc[q] == c and nw[q] == w
            assert (rows[a:b] == r).all() and (_bits(dist[a:b]) == _bits(d)).all()


@pytest.mark.parametrize("option,value", [("rerank_mode", 1), ("rerank_mode", 2), ("tile_filter", 0), ("tile_filter", 2),
                                          ("screen_i8", 0), ("screen_f16", 0), ("i8_form", 1), ("i8_form", 2),
                                          ("probe_rows", 0), ("probe_rows", 2), ("single_bucket", 0), ("single_bucket", 2),
                                          ("wide_quads", 0), ("layout", "row_order")])
def test_table_answers_under_every_searcher_option(pqv, oracle, option, value):
    rng = np.random.default_rng(21)
    dim = 256
    sizes, kcs = [3000, 1200, 2200], [8, 4, 6]
    t = Table(pqv, oracle, rng, sizes, kcs, dim, flags=pqv.PQV_LAYOUT_ROW_ORDER if option == "layout" else None)
    if option != "layout":
        t.s.set_option(option, value)
    queries = rng.random((200, dim), dtype=np.float32)
    for nq in (1, 200):
        for k in (10, 100):
            rows, dist, nf, nc = t.s.topk(queries[:nq], k, 3, sqrt_out=False)
            for q in (range(nq) if nq < 200 else range(0, 200, 23)):
                er, ed, ncand = t.expect_topk(queries[q], k, 3)
                assert nc[q] == ncand and nf[q] == len(er)
                assert (rows[q, :len(er)] == er).all() and (_bits(dist[q, :len(er)]) == _bits(ed)).all()


def test_table_limits(pqv, oracle):
    import torch
    rng = np.random.default_rng(33)
    t = Table(pqv, oracle, rng, [2600, 2600, 2600], [520, 520, 520], 8)
    nprobe = 400                                      # P = 1200 > 1024 lists per query
    queries = rng.random((2, 8), dtype=np.float32)
    rows, d2, nf, nc = t.s.topk(queries, 10, nprobe, sqrt_out=False)
    for q in range(2):
        er, ed, ncand = t.expect_topk(queries[q], 10, nprobe)
        assert nc[q] == ncand and (rows[q, :len(er)] == er).all() and (_bits(d2[q, :len(er)]) == _bits(ed)).all()
    assert len(t.s.probe(queries[0], nprobe)) == 1200
    with pytest.raises(pqv.PqvError) as e:
        _device_topk(torch, t.s, queries, 10, nprobe)
    assert e.value.code == pqv._ffi.PQV_ERR_UNSUPPORTED
    for call in (lambda: t.s.topk(queries, 10, 2, max_candidates=100),
                 lambda: t.s.range_search(queries, 1.0, 2, max_candidates=100),
                 lambda: _device_topk(torch, t.s, queries, 10, 2, max_candidates=100)):
        with pytest.raises(pqv.PqvError, match="max_candidates") as e:
            call()
        assert e.value.code == pqv._ffi.PQV_ERR_UNSUPPORTED


def test_table_builders_end_to_end(pqv, oracle, tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    rng = np.random.default_rng(77)
    dim, paths, data = 16, [], []
    for f, n in enumerate((700, 300, 1100)):
        vecs = rng.random((n, dim), dtype=np.float32)
        p = str(tmp_path / f"part{f}.parquet")
        pq.write_table(pa.table({"id": pa.array(np.arange(n, dtype=np.int64)),
                                 "vec": pa.array(vecs.tolist(), type=pa.list_(pa.float32()))}), p, row_group_size=256)
        pqv.IndexBuilder(p, "vec").n_clusters(4 + 2 * f).build_inplace()
        paths.append(p)
        data.append(vecs)
    q = rng.random(dim, dtype=np.float32)
    for k, nprobe in ((10, 2), (50, 3)):
        got = pqv.TableTopkBuilder(paths, q).k(k).nprobe(nprobe).search()
        merged = []
        for f, p in enumerate(paths):
            res = pqv.TopkBuilder(p, q).k(k).nprobe(nprobe).search()
            merged += [(r.distance, f, i, r.row_idx) for i, r in enumerate(res)]
        merged.sort()
        want = [(paths[f], row, d) for d, f, _, row in merged[:k]]
        assert [(r.path, r.row_idx) for r in got] == [(w[0], w[1]) for w in want]
        assert _bits([r.distance for r in got]).tolist() == _bits([w[2] for w in want]).tolist()
    got = pqv.TableRangeBuilder(paths, q).radius(1.2).nprobe(2).search()
    s = pqv.searcher_for_parquet_files(paths)
    _, rows, dist, _, _ = s.range_search(q.reshape(1, -1), 1.2, 2)
    f, local = s.split_rows(rows)
    assert [(r.path, r.row_idx) for r in got] == [(paths[i], int(r)) for i, r in zip(f.tolist(), local.tolist())]
    assert all(r.distance <= 1.2 for r in got)
