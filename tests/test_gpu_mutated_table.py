"""Tables whose files had rows appended, removed and compacted (pqv_table_searcher_create: a file's extent is its index' row bound).

Three files of dim 64 over one corpus, their indexes made on the GPU as tests/test_gpu_mutated_search.py makes them: file 0 is
`built`, file 1 `appended`, file 2 `removed` -- in a second table `compacted` --, row_base spaced by each file's row BOUND.  The
expectation is the per-file oracle searches over the model's lists merged by (distance, position in the file-major candidate
sequence), with mask_ref / key_filter_ref for the filters and the oracle's CandidateCursor for the round-robin quotas; split_rows
maps every returned row to its file and local id, local ids at or above the removed file's count of list rows included."""
import numpy as np
import pytest

import key_filter_ref
import mask_ref
import mutated_cases as mc
from range_oracle import REF4, l2_chain
from test_gpu_mutated_search import Zoo
from test_gpu_table_cap import _quotas

pytestmark = pytest.mark.gpu

NQ = 16


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class MutatedTable:
    def __init__(self, pqv, oracle, zoo, states, flags=None):
        from pq_vector_amd import _ffi
        self.oracle, self.case = oracle, zoo.case
        self.models = [zoo.case.models[s] for s in states]
        self.indexes = [zoo.index[s] for s in states]
        bounds = [m.bound for m in self.models]
        assert [ix.row_bound for ix in self.indexes] == bounds
        self.row_base = np.concatenate([[0], np.cumsum(bounds)[:-1]]).astype(np.uint64)
        # (the files hold the same rows: shifted a little per file, or every row of `built` would tie with its copy in `appended`)
        self.file_data = [(m.X[:b] + np.float32(f) * np.float32(2.0 ** -10)).astype(np.float32) for f, (m, b) in enumerate(zip(self.models, bounds))]
        self.data = np.ascontiguousarray(np.concatenate(self.file_data))
        self.corpus = pqv.Corpus.upload(self.data)
        flags = _ffi.PQV_LAYOUT_IVF_ORDERED | (flags or 0)
        self.s = pqv.TableSearcher(self.indexes, self.corpus, self.row_base, flags)
        self.allowed = np.concatenate([m.masks["dense"][:b] for m, b in zip(self.models, bounds)])
        self.tenant = np.ascontiguousarray(np.concatenate([m.cols["tenant"][0][:b] for m, b in zip(self.models, bounds)]))
        self.mask = self.s.row_mask(self.allowed)
        column = pqv.Column.upload(self.tenant)
        self.keys = self.s.row_keys(column)
        column.close()
        self.Q = zoo.case.Q[:NQ]
        self.qkeys = zoo.case.qkeys[:NQ]

    def close(self):
        for h in (self.mask, self.keys, self.s, self.corpus):
            h.close()

    def per_file(self, q, nprobe):
        return [m.oidx(self.oracle).candidate_rows(q, nprobe).astype(np.int64) + int(b) for m, b in zip(self.models, self.row_base)]

    def selected(self, q, nprobe, cap=0):
        """-> (the considered candidates in table order, the files' quotas, the uncapped total)"""
        lists = self.per_file(q, nprobe)
        quota = _quotas(self.oracle, lists, cap)
        return np.concatenate([x[:n] for x, n in zip(lists, quota)]).astype(np.uint32), quota, sum(len(x) for x in lists)

    def allow_for(self, i, masked, keyed):
        a = self.allowed if masked else np.ones(len(self.data), bool)
        if keyed:
            a = key_filter_ref.allowed_for(self.tenant, None, key_filter_ref.EQ, self.qkeys, None, i, a)
        return a

    def kw(self, masked, keyed):
        kw = {"mask": self.mask} if masked else {}
        if keyed:
            kw.update(keys=self.keys, query_keys=self.qkeys)
        return kw


@pytest.fixture(scope="module")
def tables(pqv, oracle):
    zoo = Zoo(pqv, oracle, "screened", searchers=False)          # the corpus that grows and the five indexes, nothing else
    made = {}

    def get(last, capped=False):
        if (last, capped) not in made:
            made[(last, capped)] = MutatedTable(pqv, oracle, zoo, ["built", "appended", last], pqv.PQV_TABLE_CAP_ROUND_ROBIN if capped else None)
        return made[(last, capped)]
    yield get
    for t in made.values():
        t.close()
    zoo.close()


@pytest.mark.parametrize("last", ["removed", "compacted"])
def test_a_table_takes_a_file_by_its_row_bound(tables, last):
    t = tables(last)
    m = t.models[2]
    assert t.s.n_rows.tolist() == [sum(len(l) for l in mm.lists) for mm in t.models]
    assert t.s.extents.tolist() == [mm.bound for mm in t.models]
    assert (t.s.extents[2] > t.s.n_rows[2]) == (last == "removed")
    assert "table of 3 files" in t.s.describe(NQ, mc.K, mc.NPROBE)
    for q in t.Q[:3]:
        assert np.array_equal(t.s.candidate_rows(q, mc.NPROBE), t.selected(q, mc.NPROBE)[0])
    # every list row of the last file maps to it, with its own id
    rows = (np.concatenate(m.lists).astype(np.int64) + int(t.row_base[2])).astype(np.uint32)
    f, local = t.s.split_rows(rows)
    assert (f == 2).all() and np.array_equal(local, np.concatenate(m.lists).astype(np.uint32))
    assert (local >= t.s.n_rows[2]).any() == (last == "removed")


@pytest.mark.parametrize("keyed", [False, True], ids=["", "keyed"])
@pytest.mark.parametrize("masked", [False, True], ids=["", "masked"])
@pytest.mark.parametrize("last", ["removed", "compacted"])
def test_table_topk_and_range_equal_the_per_file_oracle_merged(tables, last, masked, keyed):
    from test_gpu_table import _device_topk
    import torch
    t = tables(last)
    k, nprobe = mc.K, (t.case.nprobe_f if keyed else mc.NPROBE)
    kw = t.kw(masked, keyed)
    host = t.s.topk(t.Q, k, nprobe, sqrt_out=False, **kw)
    dkw = dict(kw)
    if keyed:
        qk_t = torch.from_numpy(t.qkeys).to(torch.device("cuda", 0))
        dkw["query_keys"] = qk_t.data_ptr()
    dev = _device_topk(torch, t.s, t.Q, k, nprobe, **dkw)
    in_last = above = 0
    for i, q in enumerate(t.Q):
        cand, _, total = t.selected(q, nprobe)
        rows, d2, _, _ = mask_ref.masked_topk(cand, t.allow_for(i, masked, keyed), t.data, q, k)
        for what, (grow, gd, gnf, gnc) in (("host", host), ("device", dev)):
            assert gnc[i] == total and gnf[i] == len(rows), what
            assert (grow[i, :len(rows)] == rows).all() and (_bits(gd[i, :len(rows)]) == _bits(d2)).all(), what
            assert (grow[i, len(rows):] == mc.EMPTY).all()
        f, local = t.s.split_rows(host[0][i, :len(rows)])
        assert np.array_equal(f, np.searchsorted(t.row_base, rows, side="right") - 1)
        assert np.array_equal(local.astype(np.int64), rows.astype(np.int64) - t.row_base[f].astype(np.int64))
        for ff, ll in zip(f.tolist(), local.tolist()):          # ... and the row is that file's row, one its lists hold
            assert (t.data[int(t.row_base[ff]) + ll] == t.file_data[ff][ll]).all() and t.models[ff].in_lists()[ll]
        in_last += int((f == 2).sum())
        above += int(((f == 2) & (local >= t.s.n_rows[2])).sum())
    assert in_last > 0 and (above > 0) == (last == "removed")          # local ids at or above the removed file's list-row count come back
    # range
    d_all = np.concatenate([np.sqrt(l2_chain(t.data[t.selected(q, nprobe)[0]], q, REF4)) for q in t.Q[:4]])
    radius = float(np.quantile(d_all, 0.02))
    lims, rows, dist, nw, nc = t.s.range_search(t.Q, radius, nprobe, max_results=9, **kw)
    for i, q in enumerate(t.Q):
        cand, _, total = t.selected(q, nprobe)
        r, d, w, _ = mask_ref.masked_range(cand, t.allow_for(i, masked, keyed), t.data, q, radius, max_results=9)
        a, b = int(lims[i]), int(lims[i + 1])
        assert nc[i] == total and nw[i] == w and b - a == len(r)
        assert (rows[a:b] == r).all() and (_bits(dist[a:b]) == _bits(d)).all()
    assert nw.sum() > 0 and (nw < nc).all()


@pytest.mark.parametrize("masked", [False, True], ids=["", "masked"])
@pytest.mark.parametrize("last", ["removed", "compacted"])
def test_the_round_robin_cap_cuts_into_the_mutated_file(tables, last, masked):
    t = tables(last, capped=True)
    k, nprobe, cap = mc.K, mc.NPROBE, 600
    kw = t.kw(masked, False)
    rows, d2, nf, nc = t.s.topk(t.Q, k, nprobe, max_candidates=cap, sqrt_out=False, **kw)
    # a radius with hits for every query that cuts every query's considered rows: from the model's distances over the capped selection
    ends = []
    for i, q in enumerate(t.Q):
        sel = t.selected(q, nprobe, cap)[0]
        d = np.sqrt(l2_chain(t.data[sel[t.allow_for(i, masked, False)[sel]]], q, REF4))
        ends.append((float(d.min()), float(d.max())))
    radius = mc.pick_radius(ends)
    lims, rrows, rdist, nw, rnc = t.s.range_search(t.Q, radius, nprobe, max_candidates=cap, **kw)
    cut = 0
    for i, q in enumerate(t.Q):
        sel, quota, total = t.selected(q, nprobe, cap)
        counts = [len(x) for x in t.per_file(q, nprobe)]
        cut += int(0 < quota[2] < counts[2])
        er, ed, _, _ = mask_ref.masked_topk(sel, t.allow_for(i, masked, False), t.data, q, k)
        assert nc[i] == total and nf[i] == len(er)
        assert (rows[i, :len(er)] == er).all() and (_bits(d2[i, :len(er)]) == _bits(ed)).all()
        r, d, w, _ = mask_ref.masked_range(sel, t.allow_for(i, masked, False), t.data, q, radius)
        a, b = int(lims[i]), int(lims[i + 1])
        assert rnc[i] == total and nw[i] == w and (rrows[a:b] == r).all() and (_bits(rdist[a:b]) == _bits(d)).all()
    assert cut == len(t.Q)
    assert (nw > 0).all() and (nw < cap).all() and (nw < rnc).all()


def test_a_table_of_parquet_files_keeps_a_file_after_a_delete(pqv, tmp_path):
    """The builders' path: file 1 is written again with an index that lost 40 % of its rows, the newest 25 among them, so its blob's
    bound lies below the file's row count.  Every list is probed: the answer is the exact top-k over the surviving rows, under a
    predicate over a column of the files and under per-file bool arrays too."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    from pq_vector_amd import parquet_io
    rng = np.random.default_rng(91)
    dim, n, kc, k = 16, 900, 4, 30
    data, tags, paths = [], [], []
    for f in range(2):
        data.append(rng.random((n, dim), dtype=np.float32))
        tags.append(rng.integers(0, 4, n).astype(np.int32))
        paths.append(str(tmp_path / f"part{f}.parquet"))
        pq.write_table(pa.table({"tag": pa.array(tags[f]), "vec": pa.array(data[f].tolist(), type=pa.list_(pa.float32()))}), paths[f],
                       row_group_size=256)
        pqv.IndexBuilder(paths[f], "vec").n_clusters(kc).max_iters(5).build_inplace()
    gone = rng.random(n) < 0.4
    gone[n - 25:] = True
    index, column = parquet_io.read_index_from_parquet(paths[1])
    removed = index.remove(flags=gone)
    assert removed.n_rows == int((~gone).sum()) and pqv.Index.from_bytes(removed.to_bytes()).row_bound < n
    after = str(tmp_path / "part1_after_delete.parquet")
    parquet_io.write_parquet_with_index(paths[1], after, removed, column)
    paths[1] = after
    alive = [np.ones(n, bool), ~gone]
    q = rng.random(dim, dtype=np.float32)
    per_file = [rng.random(n) < 0.5, rng.random(n) < 0.5]          # (they allow removed rows too)

    def want(allow):
        d2 = np.concatenate([l2_chain(data[f], q, REF4) for f in range(2)])
        ok = np.concatenate([alive[f] & allow[f] for f in range(2)])
        at = np.nonzero(ok)[0]
        top = at[np.lexsort((at, d2[at]))][:k]
        return [(paths[int(r) // n], int(r) % n) for r in top], np.sqrt(d2[top])

    above = 0
    for where, allow in ((None, [np.ones(n, bool)] * 2), (pqv.col("tag") >= 2, [t >= 2 for t in tags]), (per_file, per_file)):
        b = pqv.TableTopkBuilder(paths, q).k(k).nprobe(kc)
        got = (b if where is None else b.where(where)).search()
        rows, dist = want(allow)
        assert [(r.path, r.row_idx) for r in got] == rows
        assert _bits([r.distance for r in got]).tolist() == _bits(dist).tolist()
        above += sum(r.path == after and r.row_idx >= removed.n_rows for r in got)
    assert above >= 3          # ids above the count of list rows come back
    s = pqv.searcher_for_parquet_files(paths)
    assert s.n_rows.tolist() == [n, removed.n_rows] and s.extents.tolist() == [n, n] and s.row_base.tolist() == [0, n]
