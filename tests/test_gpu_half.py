"""Half-precision corpora (pqv.h): f16 rows searched by stream_h_kernel against the SAME calls on an f32 searcher over the widened
rows (exact stream, rerank_mode 1) and the CPU oracle on the widened rows -- row ids, distance BITS, n_found, n_candidates, range
CSR and counters equal, no tolerance: widening is exact.  Index: oracle-built centroids, lists re-dealt (one row, empty, multi-block)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REF4, SEQ = 0, 1
DIMS = [1, 3, 4, 7, 8, 12, 30, 72, 100, 256, 264, 516, 768]
N, KC = 3000, 12
_CASE = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _halves(rng, n, dim, ties=False):
    if ties:       # small integers: many equal distances
        return rng.integers(0, 3, size=(n, dim)).astype(np.float16)
    h = rng.standard_normal((n, dim)).astype(np.float16)
    edge = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x7BFF, 0xFBFF], dtype=np.uint16).view(np.float16)   # +-0, subnormals, +-65504
    flat = h.reshape(-1)
    flat[rng.choice(flat.size, size=min(flat.size, 8 * len(edge)), replace=False)] = np.resize(edge, min(flat.size, 8 * len(edge)))
    return h


def _case(pqv, oracle, dim, ties=False):
    """(f16 rows, widened rows, oracle index, f16 searcher, f32 reference searcher), built once per shape"""
    key = (dim, ties)
    if key not in _CASE:
        rng = np.random.default_rng(1000 + dim + (7 if ties else 0))
        h = _halves(rng, N, dim, ties)
        wide = h.astype(np.float32)
        cents = oracle.build_index(np.clip(wide, -4, 4), n_clusters=KC, workers=4).centroids
        # (any assignment of rows to lists is a valid index) reshaped: list 0 one row, list 1 empty, list 2 > 1024 rows
        near = rng.integers(0, KC, size=N)
        order = np.argsort(near, kind="stable").astype(np.uint32)
        cuts = [0, 1, 1, 1301] + list(np.linspace(1301, N, KC - 2).astype(int)[1:])
        lists = [order[cuts[i]:cuts[i + 1]] for i in range(KC)]
        oidx = oracle.index_from_parts(dim, cents, lists)
        index = pqv.Index.from_parts(dim, cents, lists)
        sh = pqv.Searcher(index, pqv.Corpus.upload(h))
        sf = pqv.Searcher(index, pqv.Corpus.upload(wide), pqv.PQV_LAYOUT_ROW_ORDER).set_option("rerank_mode", 1)
        # continuous f32 queries; a seed at which no parameter case ties among a query's k + 1 nearest (checked with the chains in numpy)
        queries = np.random.default_rng(5007 + dim).standard_normal((33, dim)).astype(np.float32)
        _CASE[key] = (h, wide, oidx, sh, sf, queries)
    return _CASE[key]


def _same_topk(got, exp):
    for g, e, what in zip(got, exp, ("rows", "dist", "n_found", "n_candidates")):
        assert (_bits(g) == _bits(e)).all() if what == "dist" else (g == e).all(), what


def _same_range(got, exp):
    for g, e, what in zip(got, exp, ("lims", "rows", "dist", "n_within", "n_candidates")):
        assert (_bits(g) == _bits(e)).all() if what == "dist" else (np.asarray(g) == np.asarray(e)).all(), what


def _device_call(s, queries, k, nprobe, flags, **kw):
    import torch
    q = torch.from_numpy(queries).cuda()
    nq = len(queries)
    rows = torch.zeros((nq, k), dtype=torch.int32, device="cuda")
    dist = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
    nf = torch.zeros(nq, dtype=torch.int32, device="cuda")
    nc = torch.zeros(nq, dtype=torch.int64, device="cuda")
    tie = torch.zeros(nq, dtype=torch.int32, device="cuda")
    s.topk_device(q.data_ptr(), nq, k, nprobe, rows.data_ptr(), dist.data_ptr(), nf.data_ptr(), nc.data_ptr(),
                  d_tie_flags=tie.data_ptr() if flags else 0, **kw)
    torch.cuda.synchronize()
    return (rows.cpu().numpy().view(np.uint32), dist.cpu().numpy(), nf.cpu().numpy().view(np.uint32), nc.cpu().numpy().view(np.uint64)), tie.cpu().numpy()


@pytest.mark.parametrize("dim", DIMS)
def test_half_dims(pqv, oracle, dim):
    """every load form and chunk count: host top-k (both metrics), the oracle, and a range search at the median candidate distance"""
    h, wide, oidx, sh, sf, queries = _case(pqv, oracle, dim)
    for nq in (1, 33):
        q = queries[:nq]
        got = sh.topk(q, 10, 5)
        _same_topk(got, sf.topk(q, 10, 5))
        _same_topk(got, oidx.topk_batch(wide, q, 10, 5))
        _same_topk(sh.topk(q, 10, 5, metric=SEQ, sqrt_out=False), sf.topk(q, 10, 5, metric=SEQ, sqrt_out=False))
    d = sf.topk(queries[:1], 300, 5)[1][0]
    radius = float(d[np.isfinite(d)][np.isfinite(d).sum() // 2])
    for metric in (REF4, SEQ):
        _same_range(sh.range_search(queries, radius, 5, metric=metric), sf.range_search(queries, radius, 5, metric=metric))
    c0h, c0f = sh.counters(), sf.counters()
    _same_range(sh.range_search(queries, np.inf, 5, max_results=7, sqrt_out=False), sf.range_search(queries, np.inf, 5, max_results=7, sqrt_out=False))
    c1h, c1f = sh.counters(), sf.counters()
    for name in ("queries", "candidate_rows", "embeddings_fetched", "exact_replays"):
        assert c1h[name] - c0h[name] == c1f[name] - c0f[name], name


@pytest.mark.parametrize("k,nprobe,metric,sqrt_out,cap", [
    (1, 5, REF4, False, 0), (100, 5, REF4, False, 0), (300, 5, REF4, False, 0), (10, 1, REF4, False, 0), (10, 64, REF4, False, 0),
    (10, 5, REF4, True, 0), (10, 5, SEQ, False, 0), (10, 5, REF4, False, 1500), (300, 64, SEQ, False, 1700), (100, 1, SEQ, True, 0)])
@pytest.mark.parametrize("dim", [30, 264])
def test_half_parameters(pqv, oracle, dim, k, nprobe, metric, sqrt_out, cap):
    """each axis against the base case (k 10, nprobe 5, REF4, d2 out: sqrt rounds neighbouring distances together at k 300) and mixed cases, host and device forms, counters included"""
    h, wide, oidx, sh, sf, queries = _case(pqv, oracle, dim)
    kw = dict(max_candidates=cap, metric=metric, sqrt_out=sqrt_out)
    c0h, c0f = sh.counters(), sf.counters()
    exp = sf.topk(queries, k, nprobe, **kw)
    _same_topk(sh.topk(queries, k, nprobe, **kw), exp)
    got, tie = _device_call(sh, queries, k, nprobe, True, **kw)
    assert (tie == 0).all(), "continuous data must not tie (a condition on the inputs)"
    _same_topk(got, exp)
    _same_topk(_device_call(sh, queries, k, nprobe, False, **kw)[0], exp)
    _same_topk(_device_call(sf, queries, k, nprobe, False, **kw)[0], exp)       # (the reference counts the same three calls)
    _device_call(sf, queries, k, nprobe, True, **kw)
    c1h, c1f = sh.counters(), sf.counters()
    for name in ("queries", "candidate_rows", "embeddings_fetched", "exact_replays"):
        assert c1h[name] - c0h[name] == c1f[name] - c0f[name], name
    assert c1h["screened_pairs"] == 0 and c1h["screen_survivors"] == 0


def test_half_ties_and_large_k(pqv, oracle):
    """equal distances: the host form replays the heap through the f16 STREAM_DIST; the device form flags them; k beyond the lists"""
    h, wide, oidx, sh, sf, queries = _case(pqv, oracle, 12, ties=True)
    q = np.round(queries).astype(np.float32)
    _same_topk(sh.topk(q, 10, 5), oidx.topk_batch(wide, q, 10, 5))
    got, tie = _device_call(sh, q, 10, 5, True)
    ref, rtie = _device_call(sf, q, 10, 5, True)
    assert tie.any() and (tie == rtie).all()
    for g, e in zip(got, ref):
        assert (_bits(g)[tie == 0] == _bits(e)[tie == 0]).all()
    h, wide, oidx, sh, sf, queries = _case(pqv, oracle, 30)
    got, exp = sh.topk(queries[:3], 1500, 5), oidx.topk_batch(wide, queries[:3], 1500, 5)
    _same_topk(got, sf.topk(queries[:3], 1500, 5))
    assert (got[2] == exp[2]).all() and (got[3] == exp[3]).all() and (got[2] < 1500).all()
    for i, nf in enumerate(got[2]):      # (behind n_found the library pads with 0xFFFFFFFF / inf, the oracle binding with zeros)
        assert (got[0][i, :nf] == exp[0][i, :nf]).all() and (_bits(got[1][i, :nf]) == _bits(exp[1][i, :nf])).all()


def test_half_corpus_plumbing(pqv, oracle):
    import torch
    h, wide, oidx, sh, sf, queries = _case(pqv, oracle, 30)
    index = pqv.Index.from_parts(30, oidx.centroids, oidx.lists())
    exp = sh.topk(queries, 10, 5)
    up = pqv.Corpus.upload(h)
    assert up.dtype == np.float16 and pqv.Corpus.upload(wide).dtype == np.float32
    ids = np.array([0, 7, N - 1, 7], dtype=np.uint32)
    assert (_bits(up.fetch_rows(ids)) == _bits(wide[ids])).all()
    streamed = pqv.Corpus.create(N + 5, 30, dtype=np.float16)
    streamed.write_rows(1000, h[1000:])
    streamed.write_rows(0, h[:1000])
    streamed.finish(N)
    appended = pqv.Corpus.create(N, 30, dtype=np.float16)
    appended.append(h[:17])
    appended.append(h[17:])
    t = torch.from_numpy(h).cuda()
    for corpus in (streamed, appended, pqv.Corpus.from_device(t)):
        assert corpus.dtype == np.float16 and corpus.rows == N
        _same_topk(pqv.Searcher(index, corpus).topk(queries, 10, 5), exp)
    f32c = pqv.Corpus.create(8, 30)
    for corpus, rows, text in ((streamed, wide[:2], "corpus rows are f16"), (streamed, wide[:2].astype(np.float64), "corpus rows are f16"),
                               (f32c, h[:2], "corpus rows are f32")):
        for call in (corpus.append, lambda r, c=corpus: c.write_rows(0, r)):
            with pytest.raises(pqv.PqvError, match=text) as e:
                call(rows)
            assert e.value.code == pqv._ffi.PQV_ERR_INVALID
    with pytest.raises(pqv.PqvError, match="corpus rows are f16"):
        streamed.write_plain_pages(0, np.zeros(1, np.uint64), np.zeros(1, np.uint32), np.zeros(1, np.uint64), np.zeros(1, np.uint32), 30, 1)
    with pytest.raises(pqv.PqvError, match="on a GPU"):
        pqv.Corpus.from_device(torch.from_numpy(h))
    assert sh.footprint()["row_order_bytes"] == N * 30 * 2 and "stream_h_kernel" in sh.describe(8, 10, 5)


class _Ctx:       # what the refused calls take: f16 searcher / corpus / index, host and device queries and outputs, keys, partition, mask
    def __init__(self, pqv, sh, h, index, queries):
        import torch
        self.p, self.s, self.c, self.ix, self.q, self.nq = pqv, sh, pqv.Corpus.upload(h), index, queries, len(queries)
        col = pqv.Column.upload(np.arange(N, dtype=np.int64) % 7)
        self.keys, self.part, self.mask = sh.row_keys(col), sh.key_partition(col), sh.row_mask(np.ones(N, dtype=np.uint8))
        self.qk, self.cand = np.arange(self.nq, dtype=np.int64) % 7, [np.arange(9)] * self.nq
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
        self.t = [dev(queries), torch.zeros((self.nq, 16), dtype=torch.int64, device="cuda"), torch.zeros((self.nq, 16), dtype=torch.int64, device="cuda"),
                  dev(self.qk), dev(np.arange(self.nq + 1, dtype=np.uint64) * 9), dev(np.tile(np.arange(9, dtype=np.uint32), self.nq))]
        self.dq, self.dr, self.dd, self.dqk, self.dl, self.dc = (t.data_ptr() for t in self.t)


REFUSED = {
    "PQV_COSINE": lambda x: x.s.topk(x.q, 5, 3, metric=x.p.PQV_COSINE),
    "PQV_DOT": lambda x: x.s.range_search(x.q, 1.0, 3, metric=x.p.PQV_DOT),
    "pqv_topk_masked": lambda x: x.s.topk(x.q, 5, 3, mask=x.mask),
    "pqv_topk_masked_device": lambda x: x.s.topk_device(x.dq, x.nq, 5, 3, x.dr, x.dd, mask=x.mask),
    "pqv_range_search_masked": lambda x: x.s.range_search(x.q, 1.0, 3, mask=x.mask),
    "pqv_topk_keyed": lambda x: x.s.topk(x.q, 5, 3, keys=x.keys, query_keys=x.qk),
    "pqv_topk_keyed_device": lambda x: x.s.topk_device(x.dq, x.nq, 5, 3, x.dr, x.dd, keys=x.keys, query_keys=x.dqk),
    "pqv_range_search_keyed": lambda x: x.s.range_search(x.q, 1.0, 3, keys=x.keys, query_keys=x.qk),
    "pqv_topk_filtered": lambda x: x.s.topk(x.q, 5, 3, keys=x.keys, query_key_ranges=(x.qk, x.qk + 1)),
    "pqv_topk_filtered_device": lambda x: x.s.topk_device(x.dq, x.nq, 5, 3, x.dr, x.dd, keys=x.keys, query_key_ranges=(x.dqk, x.dqk)),
    "pqv_range_search_filtered": lambda x: x.s.range_search(x.q, 1.0, 3, keys=x.keys, query_key_ranges=(x.qk, x.qk + 1)),
    "pqv_topk_expand": lambda x: x.s.topk(x.q, 5, 3, keys=x.keys, query_keys=x.qk, max_nprobe=6),
    "pqv_topk_expand_device": lambda x: x.s.topk_device(x.dq, x.nq, 5, 3, x.dr, x.dd, keys=x.keys, query_keys=x.dqk, max_nprobe=6),
    "pqv_topk_depth": lambda x: x.s.topk(x.q, 5, 3, max_nprobe=6, d2_ratio=1.5),
    "pqv_topk_depth_device": lambda x: x.s.topk_device(x.dq, x.nq, 5, 3, x.dr, x.dd, max_nprobe=6, d2_ratio=1.5),
    "pqv_topk_distinct": lambda x: x.s.topk_distinct(x.q, 5, 3, x.keys),
    "pqv_topk_distinct_device": lambda x: x.s.topk_distinct_device(x.dq, x.nq, 5, 3, x.keys, x.dr, x.dd),
    "pqv_topk_distinct_filtered": lambda x: x.s.topk_distinct(x.q, 5, 3, x.keys, filter_keys=x.keys, query_keys=x.qk),
    "pqv_topk_distinct_expand_device": lambda x: x.s.topk_distinct_device(x.dq, x.nq, 5, 3, x.keys, x.dr, x.dd, max_nprobe=6),
    "pqv_topk_grouped": lambda x: x.s.topk_grouped(x.q, 5, 2, 3, x.keys),
    "pqv_topk_grouped_device": lambda x: x.s.topk_grouped_device(x.dq, x.nq, 5, 2, 3, x.keys, x.dr, x.dd),
    "pqv_topk_grouped_filtered_device": lambda x: x.s.topk_grouped_device(x.dq, x.nq, 5, 2, 3, x.keys, x.dr, x.dd, filter_keys=x.keys, query_keys=x.dqk),
    "pqv_topk_grouped_expand": lambda x: x.s.topk_grouped(x.q, 5, 2, 3, x.keys, max_nprobe=6),
    "pqv_topk_partition": lambda x: x.s.topk_partition(x.q, 5, x.part, query_keys=x.qk),
    "pqv_topk_partition_device": lambda x: x.s.topk_partition_device(x.dq, x.nq, 5, x.part, x.dr, x.dd, query_keys=x.dqk),
    "pqv_range_search_partition": lambda x: x.s.range_search_partition(x.q, 1.0, x.part, query_keys=x.qk),
    "pqv_topk_partition_grouped": lambda x: x.s.topk_partition_grouped(x.q, 5, 2, x.part, x.keys, query_keys=x.qk),
    "pqv_topk_partition_grouped_device": lambda x: x.s.topk_partition_grouped_device(x.dq, x.nq, 5, 2, x.part, x.keys, x.dr, x.dd, query_keys=x.dqk),
    "pqv_topk_rows": lambda x: x.s.topk_rows(x.q, 5, x.cand),
    "pqv_topk_rows_device": lambda x: x.s.topk_rows_device(x.dq, x.nq, 5, x.dl, x.dc, x.dr, x.dd),
    "pqv_score_rows": lambda x: x.s.score_rows(x.q, x.cand),
    "pqv_score_rows_device": lambda x: x.s.score_rows_device(x.dq, x.nq, x.dl, x.dc, x.dd),
    "pqv_topk_mmr": lambda x: x.s.topk_mmr(x.q, 5, 8, 3),
    "pqv_topk_mmr_device": lambda x: x.s.topk_mmr_device(x.dq, x.nq, 5, 8, 3, x.dr, x.dd),
    "pqv_mmr_select": lambda x: x.s.mmr_select(np.tile(np.arange(8, dtype=np.uint32), (x.nq, 1)), np.ones((x.nq, 8), dtype=np.float32), 5),
    "pqv_mmr_select_device": lambda x: x.s.mmr_select_device(x.dc, x.dd, x.nq, 8, 5, x.dr, x.dd),
    "pqv_table_searcher_create": lambda x: x.p.TableSearcher([x.ix], x.c, [0]),
    "pqv_brute_topk": lambda x: x.c.brute_topk(x.q, 5),
    "pqv_index_build": lambda x: x.p.IndexBuilder(x.c).n_clusters(4).build(),
    "pqv_index_assign": lambda x: x.ix.assign(x.c),
    "pqv_index_append": lambda x: x.ix.append(x.c, 0, 1),
    "pqv_index_compact": lambda x: x.ix.compact(x.c),
}


@pytest.mark.parametrize("entry", sorted(REFUSED))
def test_half_refusals(pqv, oracle, entry):
    """every refused family, host and device form: PQV_ERR_UNSUPPORTED under the entry point's name, the searcher usable afterwards"""
    h, wide, oidx, sh, sf, queries = _case(pqv, oracle, 30)
    if "ctx" not in _CASE:
        _CASE["ctx"] = _Ctx(pqv, sh, h, pqv.Index.from_parts(30, oidx.centroids, oidx.lists()), queries[:4])
    with pytest.raises(pqv.PqvError, match=entry + " does not take f16 corpora") as e:
        REFUSED[entry](_CASE["ctx"])
    assert e.value.code == pqv._ffi.PQV_ERR_UNSUPPORTED
    _same_topk(sh.topk(queries[:4], 10, 5), sf.topk(queries[:4], 10, 5))
