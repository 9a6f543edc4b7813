"""Row-masked search on the GPU (pqv_topk_masked / pqv_topk_masked_device / pqv_range_search_masked).

The yardstick of most cases is the FILTERED-LISTS setup: with max_candidates == 0 a masked call must return, bit for bit, what the
unmasked call returns on Searcher(Index.from_parts(dim, centroids, [list intersected with the allowed rows]), same corpus) --
n_candidates excepted, which stays the unmasked call's.  Caps, tables and the paths beyond the kernels' lists are held to the
numpy restatement of tests/mask_ref.py (pinned to the C oracle by tests/test_mask_host.py)."""
import json
import math
import os

import numpy as np
import pytest

import mask_ref
from range_oracle import REF4, SEQ

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = 0xFFFFFFFF


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, exp, what=""):
    for i, (x, y) in enumerate(zip(got, exp)):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and (x.view(np.uint8) == y.view(np.uint8)).all(), f"{what}: output {i} differs"


def _device(s, q, k, nprobe, flags, mask=None, metric=0, max_candidates=0):
    """topk_device with d2 output -> (rows, dist, n_found, n_candidates, tie flags or None)"""
    import torch
    dev = torch.device("cuda", 0)
    q_t = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(dev)
    nq = len(q)
    r_t = torch.full((nq, k), -1, dtype=torch.int32, device=dev)
    d_t = torch.full((nq, k), float("inf"), dtype=torch.float32, device=dev)
    nf_t = torch.zeros(nq, dtype=torch.int32, device=dev)
    nc_t = torch.zeros(nq, dtype=torch.int64, device=dev)
    tf_t = torch.full((nq,), 7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    s.topk_device(q_t.data_ptr(), nq, k, nprobe, r_t.data_ptr(), d_t.data_ptr(), nf_t.data_ptr(), nc_t.data_ptr(), sqrt_out=False,
                  max_candidates=max_candidates, metric=metric,
                  d_tie_flags=tf_t.data_ptr() if flags else 0, **({} if mask is None else {"mask": mask}))
    torch.cuda.synchronize()
    return (r_t.cpu().numpy().view(np.uint32), d_t.cpu().numpy(), nf_t.cpu().numpy().astype(np.uint32),
            nc_t.cpu().numpy().astype(np.uint64), tf_t.cpu().numpy() if flags else None)


class Setup:
    """An oracle-built index (max_iters 5) over random rows, its searcher, and filtered-lists searchers per mask."""

    def __init__(self, pqv, oracle, n, dim, kc, seed, integer=False, flags=0, lists=None):
        rng = np.random.default_rng(seed)
        self.pqv, self.oracle, self.n, self.dim = pqv, oracle, n, dim
        self.data = (rng.integers(0, 3, (n, dim)).astype(np.float32) if integer else rng.random((n, dim), dtype=np.float32))
        self.queries = (rng.integers(0, 3, (5, dim)).astype(np.float32) if integer else rng.random((5, dim), dtype=np.float32))
        built = oracle.build_index(self.data, n_clusters=kc, max_iters=5, workers=1)
        self.centroids = built.centroids
        self.lists = [np.asarray(l, np.uint32) for l in (lists(built.lists()) if lists else built.lists())]
        self.oidx = oracle.index_from_parts(dim, self.centroids, self.lists)
        self.kc = len(self.lists)
        self.corpus = pqv.Corpus.upload(self.data)
        self.flags = flags
        self.s = pqv.Searcher(pqv.Index.from_parts(dim, self.centroids, self.lists), self.corpus, flags)
        self.rng = rng

    def filtered(self, allowed, flags=None):
        return self.pqv.Searcher(self.pqv.Index.from_parts(self.dim, self.centroids, mask_ref.filtered_lists(self.lists, allowed)),
                                 self.corpus, self.flags if flags is None else flags)

    def random_mask(self, p):
        return self.rng.random(self.n) < p

    def radius(self, nprobe, metric=0):
        """a radius (sqrt scale) that about the 40 nearest unmasked candidates of query 0 are within"""
        _, d, nf, _ = self.s.topk(self.queries[:1], 40, nprobe, metric=metric)
        return float(d[0, int(nf[0]) - 1])


def _check_against_filtered(st, allowed, ks, nprobes, metric=0, queries=None, entry_points=("topk", "device", "range")):
    """every entry point, masked on st.s == unmasked on the filtered-lists searcher (n_candidates: the unmasked call's)"""
    pqv = st.pqv
    q = st.queries if queries is None else queries
    m = st.s.row_mask(allowed)
    f = st.filtered(allowed)
    assert m.rows == st.n and m.count == int(np.asarray(allowed, bool)[np.concatenate(st.lists).astype(np.int64)].sum())
    try:
        for nprobe in nprobes:
            nc_unmasked = st.s.topk(q, 1, nprobe, metric=metric)[3]
            for k in ks:
                what = f"k={k} nprobe={nprobe}"
                if "topk" in entry_points:
                    got = st.s.topk(q, k, nprobe, metric=metric, mask=m)
                    exp = f.topk(q, k, nprobe, metric=metric)
                    _same(got[:3], exp[:3], "topk " + what)
                    assert (got[3] == nc_unmasked).all(), "n_candidates " + what
                    assert (got[2] <= k).all()
                if "device" in entry_points:
                    for flags in (False, True):
                        got = _device(st.s, q, k, nprobe, flags, mask=m, metric=metric)
                        exp = _device(f, q, k, nprobe, flags, metric=metric)
                        _same(got[:3], exp[:3], f"device flags={flags} " + what)
                        assert (got[3] == nc_unmasked).all()
                        if flags:
                            assert (got[4] == exp[4]).all(), "tie flags " + what
            if "range" in entry_points:
                r = st.radius(nprobe, metric)
                for max_results in (0, 7):
                    got = st.s.range_search(q, r, nprobe, max_results=max_results, metric=metric, mask=m)
                    exp = f.range_search(q, r, nprobe, max_results=max_results, metric=metric)
                    _same(got[:4], exp[:4], f"range max_results={max_results} nprobe={nprobe}")     # lims, rows, dist, n_within
                    assert (got[4] == nc_unmasked).all()
    finally:
        m.close()
        f.close()


SHAPES = {
    "4096x128": dict(n=4096, dim=128, kc=8, metric=0),      # CG = 32; lists of ~500 rows: several 256-row blocks, four waves per list
    "2048x256": dict(n=2048, dim=256, kc=4, metric=0),      # CG = 64
    "1500x30": dict(n=1500, dim=30, kc=6, metric=0),        # unaligned rows, scalar tail (row-order reads: dim % 4 != 0)
    "2048x32-seq": dict(n=2048, dim=32, kc=4, metric=1),    # PQV_L2SQ_SEQ: the CG = 16 SEQ instantiation
}


@pytest.fixture(scope="module", params=list(SHAPES))
def shape(request, pqv, oracle):
    c = SHAPES[request.param]
    st = Setup(pqv, oracle, c["n"], c["dim"], c["kc"], seed=11 + c["dim"])
    st.metric = c["metric"]
    return st


@pytest.mark.parametrize("sel", ["1/64", "1/2", "63/64"])
def test_masked_calls_equal_the_filtered_lists_setup(shape, sel):
    """Case 1: k in {1, 10, 100, 300} (S = 1, 4, 16), nprobe in {1, 3, all}; topk, topk_device with and without tie flags,
    range_search with and without max_results."""
    st = shape
    a, b = sel.split("/")
    allowed = st.random_mask(int(a) / int(b))
    _check_against_filtered(st, allowed, (1, 10, 100, 300), (1, 3, st.kc), metric=st.metric)


def test_window_edges(pqv, oracle):
    """Case 2: masks whose set bits sit on the edges of the kernel's 64-position windows and of a wave's range."""
    st = Setup(pqv, oracle, 4096, 128, 8, seed=3)
    q1 = st.queries[:2]
    c = int(st.oidx.find_closest_centroids(q1[0], 1)[0])      # the list query 0 probes first
    lst = st.lists[c].astype(np.int64)
    assert len(lst) > 200

    def only(positions):
        a = np.zeros(st.n, bool)
        a[lst[list(positions)]] = True
        return a
    for pos in ([63], [64], [65], [63, 64, 65], [0], [len(lst) - 1], range(10, 74), range(10, 75), range(0, 64), range(0, 65),
                range(64, 128), range(len(lst))):
        _check_against_filtered(st, only(pos), (1, 10, 100), (1, st.kc), queries=q1)
    # a batch big enough that a list is cut into few blocks: a wave's range is then 128 / 192 positions, and 64 / 65 allowed rows of
    # one range fill a chain tile exactly / leave one row for the flush
    many = np.random.default_rng(1).random((620, 128), dtype=np.float32)
    for pos in (range(10, 74), range(10, 75), range(100, 164)):
        _check_against_filtered(st, only(pos), (10,), (st.kc,), queries=many, entry_points=("topk", "range"))
    # nothing at all
    m = st.s.row_mask(np.zeros(st.n, bool))
    assert m.count == 0
    rows, dist, nf, nc = st.s.topk(st.queries, 10, 3, mask=m)
    assert (nf == 0).all() and (rows == EMPTY).all() and np.isinf(dist).all() and (dist > 0).all()
    assert (nc == st.s.topk(st.queries, 10, 3)[3]).all()
    rows, dist, nf, _, tf = _device(st.s, st.queries, 10, 3, True, mask=m)
    assert (nf == 0).all() and (rows == EMPTY).all() and np.isinf(dist).all() and (tf == 0).all()
    lims, rows, dist, nw, _ = st.s.range_search(st.queries, 100.0, 3, mask=m)
    assert (lims == 0).all() and rows.size == 0 and dist.size == 0 and (nw == 0).all()
    m.close()
    # everything: the unmasked call, bit for bit
    m = st.s.row_mask(np.ones(st.n, bool))
    assert m.count == st.n
    for k, nprobe in ((1, 1), (10, 3), (300, st.kc)):
        _same(st.s.topk(st.queries, k, nprobe, mask=m), st.s.topk(st.queries, k, nprobe), "all-true topk")
        for flags in (False, True):
            got, exp = _device(st.s, st.queries, k, nprobe, flags, mask=m), _device(st.s, st.queries, k, nprobe, flags)
            _same(got[:4], exp[:4], "all-true device")
            assert flags is False or (got[4] == exp[4]).all()
    r = st.radius(3)
    _same(st.s.range_search(st.queries, r, 3, mask=m), st.s.range_search(st.queries, r, 3), "all-true range")
    m.close()


def test_empty_and_short_lists(pqv, oracle):
    """Case 2, continued: an index with an empty list and a list shorter than 64."""
    def reshape(lists):
        lists = [np.asarray(l, np.uint32) for l in lists]
        lists[1] = np.concatenate([lists[1], lists[0]]); lists[0] = lists[0][:0]
        lists[3] = np.concatenate([lists[3], lists[2][10:]]); lists[2] = lists[2][:10]
        return lists
    st = Setup(pqv, oracle, 1500, 30, 6, seed=9, lists=reshape)
    assert len(st.lists[0]) == 0 and len(st.lists[2]) == 10
    for p in (1 / 64, 1 / 2, 1.0):
        allowed = st.random_mask(p)
        _check_against_filtered(st, allowed, (1, 10, 100), (1, 3, st.kc))
        for q in st.queries[:2]:          # ... and the restatement
            m = st.s.row_mask(allowed)
            rows, d2, nc, _ = mask_ref.masked_topk(st.oidx.candidate_rows(q, st.kc), allowed, st.data, q, 10)
            got = st.s.topk(q, 10, st.kc, sqrt_out=False, mask=m)
            n = int(got[2][0])
            assert n == len(rows) and (got[0][0, :n] == rows).all() and (_bits(got[1][0, :n]) == _bits(d2)).all() and got[3][0] == nc
            m.close()


@pytest.mark.parametrize("name", ["4096x128", "1500x30", "2048x32-seq"])
def test_max_candidates_caps_before_the_mask(pqv, oracle, name):
    """Case 3: the cap falls inside a list; the result is the restatement's -- capped first, then masked."""
    c = SHAPES[name]
    st = Setup(pqv, oracle, c["n"], c["dim"], c["kc"], seed=21)
    metric = c["metric"]
    allowed = st.random_mask(0.5)
    m = st.s.row_mask(allowed)
    before = st.s.counters()
    considered = total = 0
    for q in st.queries:
        cand = st.oidx.candidate_rows(q, 3)
        first = len(st.lists[int(st.oidx.find_closest_centroids(q, 1)[0])])
        for cap in (first + 100, 37, len(cand) + 5):
            rows, d2, nc, ncons = mask_ref.masked_topk(cand, allowed, st.data, q, 10, metric=metric, max_candidates=cap)
            got = st.s.topk(q, 10, 3, max_candidates=cap, metric=metric, sqrt_out=False, mask=m)
            n = int(got[2][0])
            assert n == len(rows) and (got[0][0, :n] == rows).all() and (_bits(got[1][0, :n]) == _bits(d2)).all() and got[3][0] == nc
            dv = _device(st.s, q.reshape(1, -1), 10, 3, False, mask=m, metric=metric, max_candidates=cap)
            assert int(dv[2][0]) == n and (dv[0][0, :n] == rows).all() and (_bits(dv[1][0, :n]) == _bits(d2)).all()
            radius = float(np.sqrt(d2[min(4, len(d2) - 1)])) if len(d2) else 1.0
            rr, rd, nw, nc2 = mask_ref.masked_range(cand, allowed, st.data, q, radius, metric=metric, max_candidates=cap)
            lims, grows, gdist, gnw, gnc = st.s.range_search(q, radius, 3, max_candidates=cap, metric=metric, mask=m)
            assert (grows == rr).all() and (_bits(gdist) == _bits(rd)).all() and gnw[0] == nw and gnc[0] == nc2 and lims[1] == len(rr)
            considered += 3 * ncons
            total += 3 * len(cand)
    after = st.s.counters()
    assert after["embeddings_fetched"] - before["embeddings_fetched"] == considered
    assert after["candidate_rows"] - before["candidate_rows"] == total
    m.close()


def test_ties_follow_the_reference_heap_under_the_mask(pqv, oracle):
    """Case 4: integer-valued data; the host form replays the reference's heap over the considered rows, the device form flags the
    same queries as on the filtered-lists setup."""
    st = Setup(pqv, oracle, 3000, 8, 6, seed=4, integer=True)
    q = np.random.default_rng(2).integers(0, 3, (24, 8)).astype(np.float32)
    for p in (1 / 8, 1 / 2):
        allowed = st.random_mask(p)
        m, f = st.s.row_mask(allowed), st.filtered(allowed)
        before = st.s.counters()["exact_replays"]
        for k, nprobe in ((5, 2), (20, st.kc), (100, 3)):
            _same(st.s.topk(q, k, nprobe, mask=m)[:3], f.topk(q, k, nprobe)[:3], f"tied host form k={k}")
            got, exp = _device(st.s, q, k, nprobe, True, mask=m), _device(f, q, k, nprobe, True)
            assert (got[4] == exp[4]).all() and got[4].any()
            # ... and the oracle's heap over the filtered sequence
            for i in range(3):
                rows_c, _ = mask_ref.considered(st.oidx.candidate_rows(q[i], nprobe), allowed)
                orows, od2 = oracle.topk_df(st.data, rows_c, q[i], k)
                hr, hd, hn, _ = st.s.topk(q[i], k, nprobe, sqrt_out=False, mask=m)
                assert int(hn[0]) == len(orows) and (hr[0, :len(orows)] == orows).all() and (_bits(hd[0, :len(orows)]) == _bits(od2)).all()
        assert st.s.counters()["exact_replays"] > before
        m.close(); f.close()


def test_layouts_and_options_never_change_a_masked_result(pqv, oracle):
    """Case 5: PQV_LAYOUT_ROW_ORDER, PQV_LAYOUT_IVF_ORDERED, rerank_mode in {0, 1, 2} with tile_filter = 2: identical answers."""
    base = Setup(pqv, oracle, 6000, 128, 8, seed=6)       # (lists of ~750 rows: the screened paths apply to the unmasked call)
    allowed = base.random_mask(0.5)
    q = np.random.default_rng(8).random((40, 128), dtype=np.float32)
    exp = None
    for flags in (pqv.PQV_LAYOUT_IVF_ORDERED, pqv.PQV_LAYOUT_ROW_ORDER):
        s = pqv.Searcher(pqv.Index.from_parts(128, base.centroids, base.lists), base.corpus, flags)
        m = s.row_mask(allowed)
        for mode in (0, 1, 2):
            s.set_option("rerank_mode", mode).set_option("tile_filter", 2)
            got = (s.topk(q, 10, 3, mask=m), _device(s, q, 10, 3, True, mask=m), s.range_search(q, base.radius(3), 3, mask=m))
            if exp is None:
                exp = got
                f = base.filtered(allowed)
                _same(got[0][:3], f.topk(q, 10, 3)[:3], "against the filtered-lists setup")
                f.close()
            for g, e in zip(got, exp):
                _same(g, e, f"layout {flags} rerank_mode {mode}")
        m.close(); s.close()


def test_table_masked_equals_the_restatement(pqv, oracle):
    """Case 6: three files with a gap between their row ranges, plain and with PQV_TABLE_CAP_ROUND_ROBIN and a cap."""
    from test_gpu_table import Table
    from test_gpu_table_cap import _selected
    rng = np.random.default_rng(12)
    for rr in (False, True):
        t = Table(pqv, oracle, rng, [900, 1400, 500], [4, 6, 3], 32, gap=5, flags=pqv.PQV_TABLE_CAP_ROUND_ROBIN if rr else None)
        allowed = rng.random(len(t.data)) < 0.4
        m = t.s.row_mask(allowed)
        assert m.rows == len(t.data)
        queries = rng.random((4, 32), dtype=np.float32)
        for nprobe in (1, 2):
            for cap in ((0, 500, 2000) if rr else (0,)):
                for q in queries:
                    cand = t.cand(q, nprobe)
                    sel = _selected(t, oracle, q, nprobe, cap)[0] if cap else cand
                    rows, d2, _, _ = mask_ref.masked_topk(sel, allowed, t.data, q, 10)
                    got = t.s.topk(q, 10, nprobe, max_candidates=cap, sqrt_out=False, mask=m)
                    n = int(got[2][0])
                    assert n == len(rows) and (got[0][0, :n] == rows).all() and (_bits(got[1][0, :n]) == _bits(d2)).all()
                    assert got[3][0] == len(cand)
                    dv = _device(t.s, q.reshape(1, -1), 10, nprobe, False, mask=m, max_candidates=cap)
                    assert int(dv[2][0]) == n and (dv[0][0, :n] == rows).all() and (_bits(dv[1][0, :n]) == _bits(d2)).all()
                    radius = float(np.sqrt(d2[min(5, len(d2) - 1)])) if len(d2) else 1.0
                    rrw, rd, nw, _ = mask_ref.masked_range(sel, allowed, t.data, q, radius)
                    lims, grows, gdist, gnw, gnc = t.s.range_search(q, radius, nprobe, max_candidates=cap, mask=m)
                    assert (grows == rrw).all() and (_bits(gdist) == _bits(rd)).all() and gnw[0] == nw and gnc[0] == len(cand)
        m.close()


def test_masked_cosine_equals_the_normalised_reference_setup(pqv, oracle):
    """Case 7: masked PQV_COSINE == masked PQV_L2SQ_REF4 (sqrt_out = 0) on the normalised rows and index, halved."""
    from test_gpu_cosine import Pair, half, normalise
    rng = np.random.default_rng(14)
    data = rng.random((2048, 64), dtype=np.float32) - 0.5
    oidx = oracle.build_index(data, n_clusters=4, max_iters=5, workers=1)
    q = rng.random((6, 64), dtype=np.float32) - 0.5
    for flags in (0, pqv.PQV_LAYOUT_ROW_ORDER, pqv.PQV_PREPARE_COSINE):
        p = Pair(pqv, data, oidx, flags)
        allowed = rng.random(len(data)) < 0.3
        ms, mr = p.s.row_mask(allowed), p.ref.row_mask(allowed)
        for k, nprobe in ((1, 1), (10, 2), (100, 4)):
            got = p.s.topk(q, k, nprobe, metric=pqv.PQV_COSINE, mask=ms)
            exp = p.ref.topk(normalise(q), k, nprobe, metric=pqv.PQV_L2SQ_REF4, sqrt_out=False, mask=mr)
            assert (got[0] == exp[0]).all() and (got[2] == exp[2]).all() and (got[3] == exp[3]).all()
            assert (_bits(got[1]) == _bits(half(exp[1]))).all()
            dv = _device(p.s, q, k, nprobe, True, mask=ms, metric=pqv.PQV_COSINE)
            de = _device(p.ref, normalise(q), k, nprobe, True, mask=mr)
            assert (dv[0] == de[0]).all() and (_bits(dv[1]) == _bits(half(de[1]))).all() and (dv[4] == de[4]).all()
        radius = float(got[1][0, min(20, int(got[2][0]) - 1)])
        g = p.s.range_search(q, radius, 2, metric=pqv.PQV_COSINE, mask=ms)
        # the reference setup's hit test is on d2: halve its distances and keep those within the radius
        lims, rows, dist, _, _ = p.ref.range_search(normalise(q), np.inf, 2, metric=pqv.PQV_L2SQ_REF4, sqrt_out=False, mask=mr)
        for i in range(len(q)):
            d = half(dist[int(lims[i]):int(lims[i + 1])])
            keep = d <= np.float32(radius)
            assert (g[1][int(g[0][i]):int(g[0][i + 1])] == rows[int(lims[i]):int(lims[i + 1])][keep]).all()
            assert (_bits(g[2][int(g[0][i]):int(g[0][i + 1])]) == _bits(d[keep])).all() and g[3][i] == keep.sum()
        ms.close(); mr.close()


def test_beyond_the_kernel_lists(pqv, oracle):
    """Case 8: nprobe > 1024 on a 1100-cluster index of 2200 x 8 rows, and k = 2000: the host paths skip disallowed rows."""
    st = Setup(pqv, oracle, 2200, 8, 1100, seed=15)
    allowed = st.random_mask(0.5)
    m = st.s.row_mask(allowed)
    before = st.s.counters()
    cons = tot = 0
    for q in st.queries[:2]:
        for k, nprobe in ((10, 1100), (2000, 1100), (2000, 40)):
            cand = st.oidx.candidate_rows(q, nprobe)
            rows, d2, nc, ncons = mask_ref.masked_topk(cand, allowed, st.data, q, k)
            assert len(np.unique(_bits(d2))) == len(d2)
            got = st.s.topk(q, k, nprobe, sqrt_out=False, mask=m)
            n = int(got[2][0])
            assert n == len(rows) == min(k, ncons) and (got[0][0, :n] == rows).all() and (_bits(got[1][0, :n]) == _bits(d2)).all()
            assert got[3][0] == nc and (got[0][0, n:] == EMPTY).all()
            cons += ncons; tot += nc
        cand = st.oidx.candidate_rows(q, 1100)
        rr, rd, nw, nc = mask_ref.masked_range(cand, allowed, st.data, q, 0.5)
        lims, grows, gdist, gnw, gnc = st.s.range_search(q, 0.5, 1100, mask=m)
        assert (grows == rr).all() and (_bits(gdist) == _bits(rd)).all() and gnw[0] == nw and gnc[0] == nc
        cons += len(mask_ref.considered(cand, allowed)[0]); tot += nc
    after = st.s.counters()
    assert after["embeddings_fetched"] - before["embeddings_fetched"] == cons
    assert after["candidate_rows"] - before["candidate_rows"] == tot
    import pq_vector_amd
    with pytest.raises(pq_vector_amd.PqvError) as e:
        _device(st.s, st.queries[:1], 10, 1100, False, mask=m)
    assert e.value.code == -5
    m.close()


def test_counters(pqv, oracle):
    """Case 9: embeddings_fetched advances by the considered rows, candidate_rows by the unmasked count -- every entry point."""
    st = Setup(pqv, oracle, 4096, 128, 8, seed=17)
    allowed = st.random_mask(0.25)
    m = st.s.row_mask(allowed)
    cons = sum(len(mask_ref.considered(st.oidx.candidate_rows(q, 3), allowed)[0]) for q in st.queries)
    tot = sum(len(st.oidx.candidate_rows(q, 3)) for q in st.queries)
    calls = (lambda: st.s.topk(st.queries, 10, 3, mask=m), lambda: _device(st.s, st.queries, 10, 3, True, mask=m),
             lambda: _device(st.s, st.queries, 10, 3, False, mask=m), lambda: st.s.range_search(st.queries, 1.0, 3, mask=m))
    for call in calls:
        before = st.s.counters()
        call()
        after = st.s.counters()
        assert after["embeddings_fetched"] - before["embeddings_fetched"] == cons
        assert after["candidate_rows"] - before["candidate_rows"] == tot
        assert after["queries"] - before["queries"] == len(st.queries)
    # the unmasked call counts as before
    before = st.s.counters()
    st.s.topk(st.queries, 10, 3)
    after = st.s.counters()
    assert after["embeddings_fetched"] - before["embeddings_fetched"] == tot == after["candidate_rows"] - before["candidate_rows"]
    m.close()


@pytest.mark.parametrize("which", [0, 1])
def test_reference_fixtures_end_to_end(pqv, tmp_path, which):
    """Case 10: the reference's two filtered integration tests through a Parquet file with an id column: the predicate runs after
    candidate pruning and before the heap, and the plan counters are the snapshot's."""
    import pyarrow as pa
    import pyarrow.compute as pc
    import pyarrow.parquet as pq
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_filter_fixtures.json")))["fixtures"][which]
    path = str(tmp_path / "t.parquet")
    vec = pa.array(fx["vectors"], type=pa.list_(pa.float32()))
    pq.write_table(pa.table({"id": pa.array(range(6), type=pa.int32()), "vec": vec}), path)
    pqv.IndexBuilder(path, "vec").build_inplace()
    b = pqv.TopkBuilder(path, [0, 0]).k(2).nprobe(64).where(pc.field("id") >= fx["id_ge"])
    s = pqv.searcher_for_parquet(path)
    before = s.counters()
    res = b.search()
    after = s.counters()
    assert [r.row_idx for r in res] == fx["ids"]
    assert after["candidate_rows"] - before["candidate_rows"] == fx["candidate_rows"]
    assert after["embeddings_fetched"] - before["embeddings_fetched"] == fx["embeddings_fetched"]
    # the same predicate as a bool array, and through the range builder (every allowed row is within a large radius)
    ok = np.arange(6) >= fx["id_ge"]
    assert [r.row_idx for r in pqv.TopkBuilder(path, [0, 0]).k(2).nprobe(64).where(ok).search()] == fx["ids"]
    hits = pqv.RangeBuilder(path, [0, 0]).radius(100.0).nprobe(64).where(pc.field("id") >= fx["id_ge"]).search()
    assert sorted(r.row_idx for r in hits) == list(range(fx["id_ge"], 6)) and [r.row_idx for r in hits[:2]] == fx["ids"]
    # a table of the file twice: one expression for both files
    tres = pqv.TableTopkBuilder([path, path], [0, 0]).k(2).nprobe(64).where(pc.field("id") >= fx["id_ge"]).search()
    assert [r.row_idx for r in tres] == [fx["ids"][0], fx["ids"][0]]
    tr = pqv.TableRangeBuilder([path, path], [0, 0]).radius(100.0).nprobe(64).where([ok, np.zeros(6, bool)]).search()
    assert sorted(r.row_idx for r in tr) == list(range(fx["id_ge"], 6))
    # without where(): the unfiltered answer
    assert [r.row_idx for r in pqv.TopkBuilder(path, [0, 0]).k(2).nprobe(64).search()][0] == 0


def test_errors_and_lifetime(pqv, oracle):
    """Case 11."""
    import ctypes as C
    import torch
    from pq_vector_amd import _ffi
    st = Setup(pqv, oracle, 1500, 30, 6, seed=19)
    other = pqv.Searcher(pqv.Index.from_parts(30, st.centroids, st.lists), st.corpus)
    allowed = st.random_mask(0.5)
    m = st.s.row_mask(allowed)
    for call in (lambda: other.topk(st.queries, 5, 2, mask=m), lambda: other.range_search(st.queries, 1.0, 2, mask=m),
                 lambda: _device(other, st.queries, 5, 2, False, mask=m)):
        with pytest.raises(pqv.PqvError, match="row mask belongs to another searcher") as e:
            call()
        assert e.value.code == -1
    # the library's own length check (the Python wrapper's is bypassed)
    lib, h = _ffi.lib(), C.c_void_p()
    buf = np.ones(st.n + 1, np.uint8)
    assert lib.pqv_row_mask_create(st.s._h, buf.ctypes.data_as(_ffi.u8p), st.n + 1, C.byref(h)) == -1
    assert f"row mask has {st.n + 1} rows, the corpus has {st.n}".encode() in lib.pqv_last_error() and not h.value
    with pytest.raises(pqv.PqvError, match=f"row mask has 7 rows, the corpus has {st.n}"):
        st.s.row_mask_device(0, 7)
    q = st.queries[0]
    rows = np.zeros(5, np.uint32); dist = np.zeros(5, np.float32)
    rc = lib.pqv_topk_masked(st.s._h, None, q.ctypes.data_as(_ffi.f32p), 1, 30, 5, 2, 0, 0, 1, rows.ctypes.data_as(_ffi.u32p),
                             dist.ctypes.data_as(_ffi.f32p), None, None)
    assert rc == -1 and b"row mask must not be NULL" in lib.pqv_last_error()
    # a mask made from a torch bool tensor's device pointer == the host-made one
    t = torch.from_numpy(allowed).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    md = st.s.row_mask_device(t.data_ptr(), st.n)
    assert md.rows == m.rows == st.n and md.count == m.count == int(allowed.sum())
    _same(st.s.topk(st.queries, 10, 3, mask=md), st.s.topk(st.queries, 10, 3, mask=m), "device-made mask")
    _same(st.s.range_search(st.queries, 1.0, 3, mask=md), st.s.range_search(st.queries, 1.0, 3, mask=m), "device-made mask, range")
    # row_mask_from_rows: allow-list and deletions
    ids = np.nonzero(allowed)[0]
    a, d = st.s.row_mask_from_rows(ids), st.s.row_mask_from_rows(np.nonzero(~allowed)[0], allow=False)
    assert a.count == d.count == m.count
    _same(st.s.topk(st.queries, 10, 3, mask=a), st.s.topk(st.queries, 10, 3, mask=m), "from_rows")
    _same(st.s.topk(st.queries, 10, 3, mask=d), st.s.topk(st.queries, 10, 3, mask=m), "from_rows, deletions")
    for x in (md, a, d):
        x.close()
    # freeing the mask before the searcher, and after it
    m.close()
    assert st.s.topk(st.queries, 3, 1)[2].tolist() == [3] * 5
    late = other.row_mask(allowed)
    other.close()
    assert late.rows == st.n
    late.close()
