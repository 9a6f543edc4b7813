"""The round-robin cap of table searchers (PQV_TABLE_CAP_ROUND_ROBIN) on the GPU.  For a query, file f considers the first t_f
of its candidates, t_f being what the oracle's CandidateCursor takes from it (access.rs:214-242); the answer is the numpy chain
over that selected set ordered by (d2, table position), and what per-file searchers capped at t_f give merged with
pqv_merge_topk.  The leak trap puts every query's nearest rows just past its files' quotas."""
import math

import numpy as np
import pytest

from range_oracle import REF4, SEQ, l2_chain, range_query
from test_gpu_table import Table, _bits, _device_topk

pytestmark = pytest.mark.gpu


def _per_file(t, q, nprobe):
    return [o.candidate_rows(q, nprobe).astype(np.int64) + b for o, b in zip(t.oidx, t.row_base)]


def _quotas(oracle, lists, m):
    taken = np.zeros(len(lists), dtype=np.int64)
    if m == 0:
        return np.array([len(x) for x in lists], dtype=np.int64)
    for f, _ in oracle.candidate_cursor_take([np.arange(len(x), dtype=np.uint32) for x in lists], int(m)):
        taken[f] += 1
    return taken


def _selected(t, oracle, q, nprobe, m):
    """(selected rows in table order, quotas, uncapped total)."""
    lists = _per_file(t, q, nprobe)
    tq = _quotas(oracle, lists, m)
    sel = np.concatenate([x[:n] for x, n in zip(lists, tq)]).astype(np.uint32)
    return sel, tq, sum(len(x) for x in lists)


def _expect(t, oracle, q, k, nprobe, m, metric=REF4):
    sel, tq, total = _selected(t, oracle, q, nprobe, m)
    d2 = l2_chain(t.data[sel], q, metric)
    order = np.lexsort((np.arange(len(sel)), d2))[:k]
    return sel[order], d2[order], total, tq


def _rr_table(pqv, oracle, rng, sizes, kcs, dim, **kw):
    return Table(pqv, oracle, rng, sizes, kcs, dim, flags=pqv.PQV_TABLE_CAP_ROUND_ROBIN, **kw)


@pytest.mark.parametrize("dim", [8, 30, 128, 768])
def test_one_file_capped_table_is_a_capped_searcher(pqv, oracle, dim):
    import torch
    rng = np.random.default_rng(300 + dim)
    n = 6000 if dim < 768 else 3000
    data = rng.random((n, dim), dtype=np.float32)
    o = oracle.build_index(data, n_clusters=24, max_iters=5, workers=1)
    corpus = pqv.Corpus.upload(data)
    plain = pqv.Searcher(pqv.Index.from_bytes(o.to_bytes()), corpus)
    table = pqv.TableSearcher([pqv.Index.from_bytes(o.to_bytes())], corpus, [0], flags=pqv.PQV_TABLE_CAP_ROUND_ROBIN)
    queries = rng.random((40, dim), dtype=np.float32)
    for m in (1, 100, 2048):
        for nq in (1, 40):
            a = plain.topk(queries[:nq], 10, 3, max_candidates=m)
            b = table.topk(queries[:nq], 10, 3, max_candidates=m)
            for x, y in zip(a, b):
                assert (np.asarray(x).view(np.uint32) == np.asarray(y).view(np.uint32)).all()
            a = _device_topk(torch, plain, queries[:nq], 10, 3, max_candidates=m)
            b = _device_topk(torch, table, queries[:nq], 10, 3, max_candidates=m)
            for x, y in zip(a, b):
                assert (np.asarray(x).view(np.uint32) == np.asarray(y).view(np.uint32)).all()
            ra = plain.range_search(queries[:nq], 0.9 * math.sqrt(dim / 6), 3, max_candidates=m)
            rb = table.range_search(queries[:nq], 0.9 * math.sqrt(dim / 6), 3, max_candidates=m)
            for x, y in zip(ra, rb):
                assert (np.asarray(x).view(np.uint8) == np.asarray(y).view(np.uint8)).all()
    ca, cb = plain.counters(), table.counters()
    for key in ("queries", "candidate_rows", "embeddings_fetched"):
        assert ca[key] == cb[key], key


@pytest.mark.parametrize("F", [3, 9])
def test_capped_table_equals_the_cursor_selection_and_per_file_search(pqv, oracle, F):
    import torch
    rng = np.random.default_rng(500 + F)
    dim = 32
    sizes = [int(x) for x in rng.integers(300, 2500, F)]
    sizes[1] = 40                                      # a file whose probed lists are shorter than its share
    kcs = [2] + [int(x) for x in rng.integers(1, 12, F - 1)]
    t = _rr_table(pqv, oracle, rng, sizes, kcs, dim)
    per_file = [pqv.Searcher(ix, pqv.Corpus.upload(d)) for ix, d in zip(t.idx, t.files)]
    nprobe = 3
    queries = rng.random((12, dim), dtype=np.float32)
    totals = [_selected(t, oracle, q, nprobe, 0)[2] for q in queries]
    tot0 = totals[0]
    assert any(len(_per_file(t, q, nprobe)[1]) < 2048 // F for q in queries)      # file 1 holds less than its share
    for m in sorted({1, F - 1, F, 100, 2048, tot0 - 1, tot0, tot0 + 5}):
        for k in (1, 10, 100):
            c0 = t.s.counters()["embeddings_fetched"]
            rows, dist, nf, nc = _device_topk(torch, t.s, queries, k, nprobe, max_candidates=m)
            assert t.s.counters()["embeddings_fetched"] - c0 == sum(min(m, x) for x in totals)
            # pqv_topk: the reference heap over the capped sequence (queries with tied distances replay it)
            hr, hd, hnf, hnc = t.s.topk(queries, k, nprobe, max_candidates=m, metric=pqv.PQV_L2SQ_SEQ, sqrt_out=False)
            for q in range(len(queries)):
                er, ed, total, tq = _expect(t, oracle, queries[q], k, nprobe, m)
                assert nc[q] == total and hnc[q] == total
                assert nf[q] == len(er) and hnf[q] == len(er)
                assert (rows[q, :len(er)] == er).all() and (_bits(dist[q, :len(er)]) == _bits(ed)).all()
                orow, od2 = oracle.topk_df(t.data, _selected(t, oracle, queries[q], nprobe, m)[0], queries[q], k)
                assert (hr[q, :len(orow)] == orow).all() and (_bits(hd[q, :len(orow)]) == _bits(od2)).all()
                # per-file searchers capped at the file's quota, merged
                pr, pd, pn = [], [], []
                for f, (s_f, b) in enumerate(zip(per_file, t.row_base)):
                    if tq[f] == 0:
                        pr.append(np.full((1, k), 0xFFFFFFFF, np.uint32)); pd.append(np.full((1, k), np.inf, np.float32))
                        pn.append(np.zeros(1, np.uint32))
                        continue
                    r, d, n_f, _ = _device_topk(torch, s_f, queries[q:q + 1], k, nprobe, max_candidates=int(tq[f]))
                    pr.append(np.where(r == 0xFFFFFFFF, r, r.astype(np.int64) + b).astype(np.uint32)); pd.append(d); pn.append(n_f)
                md, mr, _, mc = pqv.merge_topk(np.stack(pd), np.stack(pr), np.stack(pn))
                assert mc[0] == nf[q]
                assert (mr[0, :nf[q]] == rows[q, :nf[q]]).all() and (_bits(md[0, :nf[q]]) == _bits(dist[q, :nf[q]])).all()


def _trap_table(pqv, oracle, rng, dim, m, nprobe, queries):
    """Three files; for every query the rows just past each file's quota become near-duplicates of the query."""
    sizes, kcs = [2600, 1500, 2000], [6, 4, 5]
    files, oidx = [], []
    for n, kc in zip(sizes, kcs):
        d = rng.random((n, dim), dtype=np.float32)
        files.append(d)
        oidx.append(oracle.build_index(d, n_clusters=kc, max_iters=5, workers=1))
    planted = [set() for _ in sizes]
    for q in queries:
        lists = [o.candidate_rows(q, nprobe).astype(np.int64) for o in oidx]
        tq = _quotas(oracle, lists, m)
        for f, (x, n) in enumerate(zip(lists, tq)):
            for r in x[n:n + 40]:                         # the 40 candidates right behind the quota
                if int(r) not in planted[f]:
                    planted[f].add(int(r))
                    files[f][r] = q + rng.normal(0, 1e-3, dim).astype(np.float32)
    return files, oidx, planted


@pytest.mark.parametrize("option,value", [(None, None), ("rerank_mode", 1), ("rerank_mode", 2), ("tile_filter", 0),
                                          ("tile_filter", 2), ("defer", 0), ("defer", 1), ("seed_refine", 0), ("seed_refine", 1),
                                          ("wide_quads", 0), ("wide_quads", 2), ("list_once", 1), ("i8_form", 1), ("i8_form", 2),
                                          ("screen_i8", 0), ("screen_f16", 0), ("probe_rows", 0), ("probe_rows", 2)])
def test_rows_past_the_quota_never_leak_in(pqv, oracle, option, value):
    import torch
    rng = np.random.default_rng(909)
    dim, nprobe, m = 768, 3, 2048
    queries = rng.random((8, dim), dtype=np.float32)
    files, oidx, planted = _trap_table(pqv, oracle, rng, dim, m, nprobe, queries)
    assert all(len(p) >= 40 for p in planted)

    class T:
        pass
    t = T()
    t.oidx, t.row_base = oidx, [0, 2600, 4100]
    t.data = np.ascontiguousarray(np.concatenate(files))
    corpus = pqv.Corpus.upload(t.data)
    s = pqv.TableSearcher([pqv.Index.from_bytes(o.to_bytes()) for o in oidx], corpus, t.row_base,
                          flags=pqv.PQV_TABLE_CAP_ROUND_ROBIN)
    if option is not None:
        s.set_option(option, value)
    # the device path orders by (d2, position): the numpy chain over the selected set; pqv_topk replays tied queries through
    # the reference heap over the capped sequence (VectorTopKExec's, SEQ chain)
    for k in (10, 100, 1000):
        want = [_expect(t, oracle, q, k, nprobe, m) for q in queries]
        heap = [oracle.topk_df(t.data, _selected(t, oracle, q, nprobe, m)[0], q, k) for q in queries]
        for nq in (1, 8):
            rows, d2, nf, nc = _device_topk(torch, s, queries[:nq], k, nprobe, max_candidates=m)
            hr, hd, hnf, hnc = s.topk(queries[:nq], k, nprobe, max_candidates=m, metric=pqv.PQV_L2SQ_SEQ, sqrt_out=False)
            for q in range(nq):
                er, ed, total, _ = want[q]
                assert nc[q] == total and nf[q] == len(er) and hnc[q] == total and hnf[q] == len(er)
                assert (rows[q, :len(er)] == er).all() and (_bits(d2[q, :len(er)]) == _bits(ed)).all()
                orow, od2 = heap[q]
                assert (hr[q, :len(orow)] == orow).all() and (_bits(hd[q, :len(orow)]) == _bits(od2)).all()


def test_capped_table_range_search_equals_the_restatement(pqv, oracle):
    rng = np.random.default_rng(19)
    t = _rr_table(pqv, oracle, rng, [4000, 700, 2500], [4, 7, 2], 16)
    queries = rng.random((9, 16), dtype=np.float32)
    for m in (1, 5, 2048, 3000):
        for radius in (0.9, 1.3, math.inf):
            lims, rows, dist, nw, nc = t.s.range_search(queries, radius, 3, max_candidates=m)
            for q in range(len(queries)):
                sel, _, total = _selected(t, oracle, queries[q], 3, m)
                r, d, w, _ = range_query(sel, t.data, queries[q], radius)
                a, b = lims[q], lims[q + 1]
                assert nc[q] == total and nw[q] == w
                assert (rows[a:b] == r).all() and (_bits(dist[a:b]) == _bits(d)).all()


def test_capped_table_ties_follow_the_reference_heap(pqv, oracle):
    import torch
    rng = np.random.default_rng(55)
    t = _rr_table(pqv, oracle, rng, [300, 120, 500, 60], [6, 3, 9, 2], 12, integer=True)
    queries = rng.integers(0, 3, (24, 12)).astype(np.float32)
    dev = torch.device("cuda", 0)
    for m in (7, 50, 200):
        r0 = t.s.counters()["exact_replays"]
        for k in (1, 10, 100):
            rows, d2, nf, nc = t.s.topk(queries, k, 2, max_candidates=m, metric=pqv.PQV_L2SQ_SEQ, sqrt_out=False)
            flags = torch.zeros(len(queries), dtype=torch.int32, device=dev)
            rows_t = torch.zeros((len(queries), k), dtype=torch.int32, device=dev)
            dist_t = torch.zeros((len(queries), k), dtype=torch.float32, device=dev)
            q_t = torch.from_numpy(queries).to(dev)
            torch.cuda.synchronize()
            t.s.topk_device(q_t.data_ptr(), len(queries), k, 2, rows_t.data_ptr(), dist_t.data_ptr(), max_candidates=m,
                            metric=pqv.PQV_L2SQ_SEQ, sqrt_out=False, d_tie_flags=flags.data_ptr())
            torch.cuda.synchronize()
            fl = flags.cpu().numpy()
            for q in range(len(queries)):
                sel, _, total = _selected(t, oracle, queries[q], 2, m)
                orow, od2 = oracle.topk_df(t.data, sel, queries[q], k)
                n = len(orow)
                assert nc[q] == total and nf[q] == n
                assert (rows[q, :n] == orow).all() and (_bits(d2[q, :n]) == _bits(od2)).all()
                dsort = np.sort(l2_chain(t.data[sel], queries[q], SEQ))[:k + 1]
                assert bool(fl[q]) == bool(len(dsort) > 1 and (np.diff(dsort) == 0).any())
        assert t.s.counters()["exact_replays"] > r0             # the case does hold ties


def test_capped_table_beyond_1024_lists(pqv, oracle):
    import torch
    rng = np.random.default_rng(61)
    t = _rr_table(pqv, oracle, rng, [2600, 2600, 2600], [520, 520, 520], 8)
    nprobe = 400                                      # P = 1200 > 1024 lists per query
    queries = rng.random((2, 8), dtype=np.float32)
    for m in (100, 2048):
        rows, d2, nf, nc = t.s.topk(queries, 10, nprobe, max_candidates=m, sqrt_out=False)
        for q in range(2):
            er, ed, total, _ = _expect(t, oracle, queries[q], 10, nprobe, m)
            assert nc[q] == total and nf[q] == len(er)
            assert (rows[q, :len(er)] == er).all() and (_bits(d2[q, :len(er)]) == _bits(ed)).all()
        lims, rr, dd, nw, nc2 = t.s.range_search(queries, 0.3, nprobe, max_candidates=m)
        for q in range(2):
            sel, _, total = _selected(t, oracle, queries[q], nprobe, m)
            r, d, w, _ = range_query(sel, t.data, queries[q], 0.3)
            assert nc2[q] == total and nw[q] == w and (rr[lims[q]:lims[q + 1]] == r).all()
        with pytest.raises(pqv.PqvError) as e:
            _device_topk(torch, t.s, queries, 10, nprobe, max_candidates=m)
        assert e.value.code == pqv._ffi.PQV_ERR_UNSUPPORTED


def test_capped_table_builder_end_to_end(pqv, oracle, tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    rng = np.random.default_rng(78)
    dim, paths, data = 16, [], []
    for f, n in enumerate((3000, 1200, 4000)):
        vecs = rng.random((n, dim), dtype=np.float32)
        p = str(tmp_path / f"part{f}.parquet")
        pq.write_table(pa.table({"id": pa.array(np.arange(n, dtype=np.int64)),
                                 "vec": pa.array(vecs.tolist(), type=pa.list_(pa.float32()))}), p, row_group_size=512)
        pqv.IndexBuilder(p, "vec").n_clusters(4 + f).build_inplace()
        paths.append(p)
        data.append(vecs)
    oidx = [oracle.index_from_bytes(pqv.read_index_from_parquet(p)[0].to_bytes()) for p in paths]
    q = rng.random(dim, dtype=np.float32)
    for k, nprobe, m in ((10, 2, 2048), (50, 3, 2048), (20, 3, 100)):
        lists = [o.candidate_rows(q, nprobe).astype(np.int64) for o in oidx]
        assert sum(len(x) for x in lists) > m
        picked = oracle.candidate_cursor_take(lists, m)
        ent = []
        for pos_f in range(len(paths)):
            rows_f = [r for f, r in picked if f == pos_f]
            d2 = l2_chain(data[pos_f][np.asarray(rows_f, dtype=np.int64)], q, REF4) if rows_f else np.zeros(0, np.float32)
            ent += [(float(d), pos_f, i, r) for i, (r, d) in enumerate(zip(rows_f, d2))]
        ent.sort()                                     # (d2, file, index in file) == (d2, table position)
        want = [(paths[f], r, np.sqrt(np.float32(d))) for d, f, _, r in ent[:k]]
        got = pqv.TableTopkBuilder(paths, q).k(k).nprobe(nprobe).max_candidates(m).search()
        assert [(r.path, r.row_idx) for r in got] == [(w[0], w[1]) for w in want]
        assert _bits([r.distance for r in got]).tolist() == _bits([w[2] for w in want]).tolist()
    got = pqv.TableRangeBuilder(paths, q).radius(0.8).nprobe(2).max_candidates(300).search()
    s = pqv.searcher_for_parquet_files(paths, round_robin_cap=True)
    _, rows, dist, _, _ = s.range_search(q.reshape(1, -1), 0.8, 2, max_candidates=300)
    f, local = s.split_rows(rows)
    assert [(r.path, r.row_idx) for r in got] == [(paths[i], int(r)) for i, r in zip(f.tolist(), local.tolist())]
    # the uncapped table of the same files is a different cache entry and still refuses a cap
    with pytest.raises(pqv.PqvError, match="max_candidates"):
        pqv.searcher_for_parquet_files(paths).topk(q.reshape(1, -1), 5, 2, max_candidates=10)
