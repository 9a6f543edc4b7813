"""PQV_DOT through the index on the GPU (include/pqv.h: PQV_DOT).  Every case is compared with the numpy model of
tests/dot_ref.py (pinned to the C oracle's chain and the summation bound by tests/test_dot_host.py): rows, distance BITS,
n_found, n_candidates, lims and n_within.  Indexes come from Index.from_parts with random centroids and a random partition of
the rows; data is finite, centred normal (dots of both signs: both branches of the key transform) or uniform [0, 1) (every
distance negative)."""
import math

import numpy as np
import pytest

import dot_ref
from test_gpu_table import Table

pytestmark = pytest.mark.gpu

EMPTY = 0xFFFFFFFF
INF_BITS = 0x7F800000
LIMIT_TEXT = "PQV_DOT takes k <= 1024 and at most 1024 probed lists per query"
KEYED_TEXT = "PQV_DOT is not supported by keyed and distinct calls"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _gen(rng, kind, shape):
    if kind == "normal":
        return rng.standard_normal(shape).astype(np.float32)
    if kind == "uniform":
        return rng.random(shape, dtype=np.float32)
    return rng.integers(-3, 4, shape).astype(np.float32)              # "integer": many exact ties


class Setup:
    def __init__(self, pqv, n, dim, kc, kind, seed, flags=0, nq=64, lens=None):
        rng = np.random.default_rng(seed)
        self.pqv, self.n, self.dim, self.kc, self.rng = pqv, n, dim, kc, rng
        self.data = _gen(rng, kind, (n, dim))
        self.queries = _gen(rng, kind, (nq, dim))
        self.centroids = _gen(rng, kind, (kc, dim))
        if lens is None:
            assign = rng.integers(0, kc, n)
            self.lists = [np.nonzero(assign == c)[0].astype(np.uint32) for c in range(kc)]
        else:                                                            # given list lengths over a random permutation of the rows
            perm = rng.permutation(n).astype(np.uint32)
            cuts = np.concatenate([[0], np.cumsum(lens)])
            assert cuts[-1] == n
            self.lists = [np.sort(perm[cuts[c]:cuts[c + 1]]) for c in range(kc)]
        self.corpus = pqv.Corpus.upload(self.data)
        self.s = self.searcher(flags)

    def searcher(self, flags=0, lists=None):
        return self.pqv.Searcher(self.pqv.Index.from_parts(self.dim, self.centroids, self.lists if lists is None else lists), self.corpus, flags)

    def m_topk(self, q, k, nprobe, **kw):
        return dot_ref.topk_batch(q, self.centroids, self.lists, self.data, k, nprobe, **kw)

    def m_range(self, q, radius, nprobe, **kw):
        return dot_ref.range_batch(q, self.centroids, self.lists, self.data, radius, nprobe, **kw)


def _same_topk(got, exp, what=""):
    rows, dist, nf, nc = got[:4]
    erows, edist, enf, enc = exp
    assert (np.asarray(nf) == enf).all(), what + " n_found"
    assert (np.asarray(nc) == enc).all(), what + " n_candidates"
    assert (np.asarray(rows) == erows).all(), what + " row ids"
    assert (_bits(dist) == _bits(edist)).all(), what + " distance bits"


def _same_range(got, exp, what=""):
    lims, rows, dist, nw, nc = got
    elims, erows, edist, enw, enc = exp
    assert (nc == enc).all(), what + " n_candidates"
    assert (nw == enw).all(), what + " n_within"
    assert (lims == elims).all(), what + " lims"
    assert (rows == erows).all(), what + " rows"
    assert (_bits(dist) == _bits(edist)).all(), what + " distance bits"


def _device(s, q, k, nprobe, flags=False, mask=None, max_candidates=0, metric=4, stream=None, q_t=None):
    """topk_device on a stream of its own -> (rows, dist, n_found, n_candidates, tie flags); q_t: queries already on the device"""
    import torch
    dev = torch.device("cuda", 0)
    if q_t is None:
        q_t = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(dev)
    nq = q_t.shape[0]
    r_t = torch.full((nq, k), -1, dtype=torch.int32, device=dev)
    d_t = torch.full((nq, k), float("nan"), dtype=torch.float32, device=dev)
    nf_t = torch.zeros(nq, dtype=torch.int32, device=dev)
    nc_t = torch.zeros(nq, dtype=torch.int64, device=dev)
    tf_t = torch.full((nq,), 7, dtype=torch.int32, device=dev)
    st = stream if stream is not None else torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        s.topk_device(q_t.data_ptr(), nq, k, nprobe, r_t.data_ptr(), d_t.data_ptr(), nf_t.data_ptr(), nc_t.data_ptr(),
                      max_candidates=max_candidates, metric=metric, sqrt_out=True, stream=st.cuda_stream,
                      d_tie_flags=tf_t.data_ptr() if flags else 0, **({} if mask is None else {"mask": mask}))
    st.synchronize()
    return (r_t.cpu().numpy().view(np.uint32), d_t.cpu().numpy(), nf_t.cpu().numpy().astype(np.uint32),
            nc_t.cpu().numpy().astype(np.uint64), tf_t.cpu().numpy())


def _check_all_topk_forms(st, q, k, nprobe, max_candidates=0):
    DOT = st.pqv.PQV_DOT
    exp = st.m_topk(q, k, nprobe, max_candidates=max_candidates)
    _same_topk(st.s.topk(q, k, nprobe, max_candidates=max_candidates, metric=DOT), exp, "topk")
    for flags in (False, True):
        got = _device(st.s, q, k, nprobe, flags, max_candidates=max_candidates)
        _same_topk(got, exp, f"device flags={flags}")
        assert (got[4] == (0 if flags else 7)).all(), "tie flags are written with zeros"
    return exp


# ---- 1. shapes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["normal", "uniform"])
@pytest.mark.parametrize("dim", [3, 8, 30, 128, 768, 1536])
def test_shapes(pqv, dim, kind):
    """tails, unaligned rows, CG 32 / 64; 64 queries and one; topk, capped topk, device forms with and without flags, range"""
    DOT = pqv.PQV_DOT
    n = 3000 if dim >= 768 else 4000
    st = Setup(pqv, n, dim, 12, kind, 1000 + dim)
    q = st.queries
    k, nprobe = 10, 3
    exp = _check_all_topk_forms(st, q, k, nprobe)
    if kind == "uniform":
        assert (exp[1] < 0).all()
    elif dim >= 30:
        assert (exp[1] < 0).any()
    _check_all_topk_forms(st, q[:1], k, nprobe)
    _same_topk(st.s.topk(q, k, nprobe, max_candidates=500, metric=DOT), st.m_topk(q, k, nprobe, max_candidates=500), "capped")
    radius = float(st.m_topk(q[:1], 41, nprobe)[1][0, 40])               # query 0's 41st distance
    got = st.s.range_search(q, radius, nprobe, metric=DOT)
    _same_range(got, st.m_range(q, radius, nprobe), "range")
    assert got[3][0] >= 41 and (got[2] <= np.float32(radius)).all()
    _same_range(st.s.range_search(q, radius, nprobe, metric=DOT, max_results=5), st.m_range(q, radius, nprobe, max_results=5), "range max_results")
    _same_range(st.s.range_search(q, radius, nprobe, metric=DOT, max_candidates=300), st.m_range(q, radius, nprobe, max_candidates=300),
                "range capped")
    _same_range(st.s.range_search(q[:1], radius, nprobe, metric=DOT), st.m_range(q[:1], radius, nprobe), "range, one query")
    if dim == 8:                                                         # mixed data: the three kinds of radius
        for r in (-0.8, 0.0, math.inf):
            _same_range(st.s.range_search(q[:8], r, nprobe, metric=DOT), st.m_range(q[:8], r, nprobe), f"radius {r}")


# ---- 2. k regimes ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def k_setup(pqv):
    return Setup(pqv, 6000, 32, 8, "normal", 2000, nq=6)


@pytest.mark.parametrize("k", [64, 65, 256, 257, 1024])
def test_k_regimes(pqv, k_setup, k):
    st = k_setup
    exp = st.m_topk(st.queries, k, 8)
    assert (exp[2] == k).all()
    _same_topk(st.s.topk(st.queries, k, 8, metric=pqv.PQV_DOT), exp, "topk")
    _same_topk(_device(st.s, st.queries, k, 8), exp, "device")
    if k < 1024:
        got = _device(st.s, st.queries, k, 8, flags=True)
        _same_topk(got, exp, "device flags")
        assert (got[4] == 0).all()


def test_fewer_candidates_than_k(pqv):
    st = Setup(pqv, 40, 32, 5, "normal", 2001, nq=4)
    exp = st.m_topk(st.queries, 64, 2)
    assert (exp[2] < 64).all()
    for got in (st.s.topk(st.queries, 64, 2, metric=pqv.PQV_DOT), _device(st.s, st.queries, 64, 2), _device(st.s, st.queries, 64, 2, flags=True)):
        _same_topk(got, exp)
        for i in range(4):
            assert (got[0][i, got[2][i]:] == EMPTY).all() and (_bits(got[1][i, got[2][i]:]) == INF_BITS).all()


# ---- 3. list geometry --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["normal", "uniform"])
def test_list_geometry(pqv, kind):
    lens = [0, 1, 63, 64, 65, 255, 256, 257, 1025]
    st = Setup(pqv, sum(lens), 16, len(lens), kind, 3000, nq=16, lens=lens)
    for nprobe in (1, 4, 9, 40):                                         # 40 > n_clusters
        _check_all_topk_forms(st, st.queries, 10, nprobe)
        _same_range(st.s.range_search(st.queries, 0.0, nprobe, metric=pqv.PQV_DOT), st.m_range(st.queries, 0.0, nprobe), f"range nprobe {nprobe}")
    _check_all_topk_forms(st, st.queries, 300, 9, max_candidates=1000)


# ---- 4. ties and zeros -------------------------------------------------------------------------------------------------
def test_ties_and_zeros(pqv):
    st = Setup(pqv, 4000, 8, 6, "integer", 4000, nq=12)
    q = st.queries.copy()
    q[0] = 0.0                                                           # a zero query: every distance +0.0f, position order
    before = st.s.counters()["exact_replays"]
    exp = _check_all_topk_forms(st, q, 50, 3)
    assert st.s.counters()["exact_replays"] == before
    assert (_bits(exp[1][0]) == 0).all()
    cand0 = dot_ref.candidates(q[0], st.centroids, st.lists, 3)
    assert (exp[0][0] == cand0[:50]).all()                               # equal distances come back in position order
    assert min(len(np.unique(d)) for d in exp[1]) < 25                   # many exact ties in every query
    got = st.s.topk(q, 50, 3, metric=pqv.PQV_DOT)
    zero = got[1] == 0
    assert zero.any() and (_bits(got[1][zero]) == 0).all()               # zero distances have bits 0
    _same_range(st.s.range_search(q, 0.0, 3, metric=pqv.PQV_DOT), st.m_range(q, 0.0, 3), "range radius 0")
    _same_range(st.s.range_search(q, -5.0, 3, metric=pqv.PQV_DOT, max_results=9), st.m_range(q, -5.0, 3, max_results=9), "range radius -5")


# ---- 5. layouts and options --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [30, 96, 128])
def test_layouts_and_options(pqv, dim):
    """flags 0 and PQV_LAYOUT_ROW_ORDER, option sets; 96 dims: the IVF copy stores the rows zero-padded to 128"""
    DOT = pqv.PQV_DOT
    st = Setup(pqv, 6000, dim, 12, "normal", 5000 + dim)
    exp = st.m_topk(st.queries, 10, 4)
    rexp = st.m_range(st.queries[:8], -1.0, 4)
    for flags in (0, pqv.PQV_LAYOUT_ROW_ORDER):
        s = st.searcher(flags)
        for opts in ({}, {"rerank_mode": 1}, {"rerank_mode": 2, "tile_filter": 2}, {"tile_filter": 0, "screen_i8": 0, "probe_rows": 2}):
            for name, value in opts.items():
                s.set_option(name, value)
            _same_topk(s.topk(st.queries, 10, 4, metric=DOT), exp, f"flags {flags} {opts}")
            _same_topk(_device(s, st.queries, 10, 4), exp, f"device flags {flags} {opts}")
            _same_range(s.range_search(st.queries[:8], -1.0, 4, metric=DOT), rexp, f"range flags {flags} {opts}")
            assert "dot_stream_kernel" in s.describe(64, 10, 4, DOT)
        s.close()


def test_images_only_layout(pqv):
    """lists of >= 192 rows of a multiple of 64 dims: the searcher keeps no f32 copy of its own and DOT reads the caller's rows"""
    st = Setup(pqv, 4000, 128, 8, "normal", 5500, nq=16)
    _check_all_topk_forms(st, st.queries, 10, 3)


# ---- 6. masks ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[30, 128, 256])
def mask_setup(request, pqv):
    return Setup(pqv, 5000, request.param, 10, "normal", 6000 + request.param, nq=16)


def _masked(st, allowed, k, nprobe, radius, max_candidates=0, filtered=True):
    DOT = st.pqv.PQV_DOT
    q = st.queries
    allow = np.asarray(allowed, bool)
    m = st.s.row_mask(allow.astype(np.uint8))
    try:
        exp = st.m_topk(q, k, nprobe, max_candidates=max_candidates, allow=allow)
        _same_topk(st.s.topk(q, k, nprobe, max_candidates=max_candidates, metric=DOT, mask=m), exp, "masked topk")
        for flags in (False, True):
            got = _device(st.s, q, k, nprobe, flags, mask=m, max_candidates=max_candidates)
            _same_topk(got, exp, "masked device")
            assert (got[4] == (0 if flags else 7)).all()
        rexp = st.m_range(q, radius, nprobe, max_candidates=max_candidates, allow=allow)
        _same_range(st.s.range_search(q, radius, nprobe, max_candidates=max_candidates, metric=DOT, mask=m), rexp, "masked range")
        _same_range(st.s.range_search(q, radius, nprobe, max_candidates=max_candidates, max_results=3, metric=DOT, mask=m),
                    st.m_range(q, radius, nprobe, max_candidates=max_candidates, max_results=3, allow=allow), "masked range max_results")
        if filtered and not max_candidates:
            # == the unmasked DOT call over from_parts(list ∩ allowed), n_candidates excepted
            f = st.searcher(lists=[l[allow[l.astype(np.int64)]] for l in st.lists])
            ft = f.topk(q, k, nprobe, metric=DOT)
            _same_topk(ft[:3] + (exp[3],), exp, "filtered lists")
            fr = f.range_search(q, radius, nprobe, metric=DOT)
            _same_range(fr[:4] + (rexp[4],), rexp, "filtered lists range")
            f.close()
        return exp
    finally:
        m.close()


def test_masks(pqv, mask_setup):
    DOT = pqv.PQV_DOT
    st = mask_setup
    q, rng = st.queries, np.random.default_rng(7)
    radius = float(st.m_topk(q[:1], 41, 4)[1][0, 40])
    ones = np.ones(st.n, bool)
    exp = _masked(st, ones, 10, 4, radius)
    _same_topk(st.s.topk(q, 10, 4, metric=DOT), exp, "all-ones mask == unmasked")
    _masked(st, rng.random(st.n) < 0.5, 10, 4, radius)
    _masked(st, rng.random(st.n) < 1 / 64, 10, 4, radius)
    _masked(st, rng.random(st.n) < 0.5, 100, 10, radius)                 # S = 4, every list
    exp = _masked(st, np.zeros(st.n, bool), 10, 4, radius)
    assert (exp[2] == 0).all()
    _masked(st, rng.random(st.n) < 0.5, 10, 4, radius, max_candidates=700)      # the cap before the mask


def test_predicate_mask(pqv, mask_setup):
    DOT = pqv.PQV_DOT
    st = mask_setup
    tenant = (np.arange(st.n) * 7919 % 13).astype(np.int32)
    st.s.attach_column("tenant", tenant)
    m = st.s.row_mask(pqv.col("tenant") >= 9)
    allow = tenant >= 9
    assert m.count == int(allow.sum())
    _same_topk(st.s.topk(st.queries, 10, 4, metric=DOT, mask=m), st.m_topk(st.queries, 10, 4, allow=allow), "predicate mask")
    _same_range(st.s.range_search(st.queries, 0.0, 4, metric=DOT, mask=m), st.m_range(st.queries, 0.0, 4, allow=allow), "predicate mask range")
    m.close()


# ---- 7. table ----------------------------------------------------------------------------------------------------------
def test_table(pqv, oracle):
    DOT = pqv.PQV_DOT
    rng = np.random.default_rng(7000)
    dim = 16
    t = Table(pqv, oracle, rng, [1500, 900], [6, 9], dim)
    files = [(np.asarray(o.centroids, np.float32).reshape(-1, dim), o.lists(), b) for o, b in zip(t.oidx, t.row_base)]
    q = (rng.random((20, dim), dtype=np.float32) - np.float32(0.5))
    for nprobe in (1, 3, 8, 20):                                         # 8: all of file 0's lists, not all of file 1's
        exp = dot_ref.topk_batch(q, None, None, t.data, 10, nprobe, files=files)
        _same_topk(t.s.topk(q, 10, nprobe, metric=DOT), exp, f"table topk nprobe {nprobe}")
        _same_topk(_device(t.s, q, 10, nprobe, flags=True), exp, f"table device nprobe {nprobe}")
        _same_topk(t.s.topk(q[:1], 10, nprobe, metric=DOT), tuple(x[:1] for x in exp), "table, one query")
        rexp = dot_ref.range_batch(q, None, None, t.data, -0.5, nprobe, files=files)
        _same_range(t.s.range_search(q, -0.5, nprobe, metric=DOT), rexp, f"table range nprobe {nprobe}")
    assert "dot_stream_kernel with one list per file" in t.s.describe(20, 10, 3, DOT)


# ---- 8. no interference ------------------------------------------------------------------------------------------------
def test_dot_leaves_l2_and_cosine_alone_and_counts_like_l2(pqv):
    DOT = pqv.PQV_DOT
    st = Setup(pqv, 4000, 128, 8, "normal", 8000, nq=32)
    s, q = st.s, st.queries

    def others():
        return (s.topk(q, 10, 3), s.topk(q, 10, 3, metric=pqv.PQV_COSINE), _device(s, q, 10, 3, metric=pqv.PQV_L2SQ_REF4)[:4],
                s.range_search(q[:4], 12.0, 3))

    a = others()
    fp1 = s.footprint()                                                  # (the cosine layout is built by now)
    c0 = s.counters()
    _check_all_topk_forms(st, q, 10, 3)
    s.range_search(q, 0.0, 3, metric=DOT)
    fp2 = s.footprint()                                                  # no layout is built for DOT
    assert all(fp2[name] == fp1[name] for name in ("row_order_bytes", "ivf_rows_bytes", "blocked_bytes"))
    c1 = s.counters()
    assert c1["screened_pairs"] == c0["screened_pairs"] and c1["screen_survivors"] == c0["screen_survivors"]
    assert c1["exact_replays"] == c0["exact_replays"]
    b = others()
    for x, y in zip(a, b):
        for u, v in zip(x, y):
            assert (np.asarray(u).view(np.uint8) == np.asarray(v).view(np.uint8)).all()

    # counters of a DOT call == the same-shape L2 call's (every list probed: the same candidates whatever the probe order)
    def delta(call):
        c_a = s.counters()
        call()
        c_b = s.counters()
        return {name: c_b[name] - c_a[name] for name in ("queries", "candidate_rows", "embeddings_fetched")}

    s.set_option("rerank_mode", 1)
    for cap in (0, 1500):
        exp_nc = st.m_topk(q, 10, 8, max_candidates=cap)[3]
        want = {"queries": len(q), "candidate_rows": int(exp_nc.sum()),
                "embeddings_fetched": int(np.minimum(exp_nc, cap).sum()) if cap else int(exp_nc.sum())}
        assert delta(lambda: s.topk(q, 10, 8, max_candidates=cap, metric=DOT)) == want
        assert delta(lambda: s.topk(q, 10, 8, max_candidates=cap)) == want
        assert delta(lambda: _device(s, q, 10, 8, max_candidates=cap)) == want
        assert delta(lambda: s.range_search(q, 0.0, 8, max_candidates=cap, metric=DOT)) == want
        assert delta(lambda: s.range_search(q, 1.0, 8, max_candidates=cap)) == want
    # masked: the considered rows are counted.  Uncapped, DOT and L2 consider the same rows; under a cap the first positions
    # depend on the probe order, which is the metric's own: the DOT call is held to the model
    allow = np.random.default_rng(8).random(st.n) < 0.5
    m = s.row_mask(allow.astype(np.uint8))
    want = {"queries": len(q), "candidate_rows": 4000 * len(q), "embeddings_fetched": int(allow.sum()) * len(q)}
    assert delta(lambda: s.topk(q, 10, 8, metric=DOT, mask=m)) == want
    assert delta(lambda: s.topk(q, 10, 8, mask=m)) == want
    assert delta(lambda: s.range_search(q, 0.0, 8, metric=DOT, mask=m)) == want
    considered = sum(int(allow[dot_ref.candidates(x, st.centroids, st.lists, 8)[:1500].astype(np.int64)].sum()) for x in q)
    want["embeddings_fetched"] = considered
    assert delta(lambda: s.topk(q, 10, 8, max_candidates=1500, metric=DOT, mask=m)) == want
    assert delta(lambda: _device(s, q, 10, 8, max_candidates=1500, mask=m)) == want
    m.close()


# ---- 9. limits and refusals --------------------------------------------------------------------------------------------
def test_limits_and_refusals(pqv):
    DOT = pqv.PQV_DOT
    UNSUPPORTED = pqv._ffi.PQV_ERR_UNSUPPORTED
    st = Setup(pqv, 2200, 8, 1100, "normal", 9000, nq=3)
    q = st.queries

    def refused(call, text, code=UNSUPPORTED):
        with pytest.raises(pqv.PqvError) as e:
            call()
        assert e.value.code == code and text in str(e.value), str(e.value)

    refused(lambda: st.s.topk(q, 1025, 4, metric=DOT), LIMIT_TEXT)
    refused(lambda: _device(st.s, q, 1025, 4), LIMIT_TEXT)
    refused(lambda: st.s.topk(q, 10, 1100, metric=DOT), LIMIT_TEXT)
    refused(lambda: _device(st.s, q, 10, 1100), LIMIT_TEXT)
    refused(lambda: st.s.range_search(q, 0.0, 1100, metric=DOT), LIMIT_TEXT)
    refused(lambda: st.s.describe(3, 1025, 4, DOT), LIMIT_TEXT)
    m = st.s.row_mask(np.ones(st.n, np.uint8))
    refused(lambda: st.s.topk(q, 10, 1100, metric=DOT, mask=m), LIMIT_TEXT)
    refused(lambda: st.s.range_search(q, 0.0, 1100, metric=DOT, mask=m), LIMIT_TEXT)
    refused(lambda: _device(st.s, q, 1025, 4, mask=m), LIMIT_TEXT)
    # at the limits the call works: k = 1024, 1024 probed lists
    _same_topk(st.s.topk(q, 1024, 1024, metric=DOT), st.m_topk(q, 1024, 1024), "k = 1024, 1024 lists")
    _same_range(st.s.range_search(q, 0.0, 1024, metric=DOT), st.m_range(q, 0.0, 1024), "range, 1024 lists")
    # keyed and distinct calls
    import torch
    keys = st.s.row_keys(pqv.Column.upload((np.arange(st.n) % 7).astype(np.int32)))
    qk = np.zeros(len(q), np.int64)
    qk_t = torch.zeros(len(q), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    refused(lambda: st.s.topk(q, 5, 3, metric=DOT, keys=keys, query_keys=qk), KEYED_TEXT)
    refused(lambda: st.s.topk(q, 5, 3, metric=DOT, keys=keys, query_keys=qk, mask=m), KEYED_TEXT)
    refused(lambda: st.s.range_search(q, 0.0, 3, metric=DOT, keys=keys, query_keys=qk), KEYED_TEXT)
    refused(lambda: st.s.topk_distinct(q, 5, 3, keys, metric=DOT), KEYED_TEXT)
    dev = torch.device("cuda", 0)
    q_t = torch.from_numpy(q).to(dev)
    r_t = torch.zeros((len(q), 5), dtype=torch.int32, device=dev)
    d_t = torch.zeros((len(q), 5), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    refused(lambda: st.s.topk_device(q_t.data_ptr(), len(q), 5, 3, r_t.data_ptr(), d_t.data_ptr(), metric=DOT, keys=keys,
                                     query_keys=qk_t.data_ptr()), KEYED_TEXT)
    refused(lambda: st.s.topk_distinct_device(q_t.data_ptr(), len(q), 5, 3, keys, r_t.data_ptr(), d_t.data_ptr(), metric=DOT), KEYED_TEXT)
    keys.close()
    m.close()
    # the re-rank entry points keep their metric check
    refused(lambda: pqv.rerank_batch(q[0], st.data[:50], 5, metric=DOT), "unknown metric", pqv._ffi.PQV_ERR_INVALID)
    refused(lambda: st.s.topk(q, 5, 3, metric=5), "unknown metric", pqv._ffi.PQV_ERR_INVALID)


# ---- 10. stream order --------------------------------------------------------------------------------------------------
def test_device_form_is_ordered_on_the_callers_stream(pqv):
    import torch
    st = Setup(pqv, 4000, 128, 12, "normal", 10000, nq=64)
    dev = torch.device("cuda", 0)
    base = torch.from_numpy(st.queries).to(dev)
    q_t = torch.zeros_like(base)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        q_t.copy_(base)
        q_t.mul_(2.0)                                                    # written on `side`, immediately before the call
    got = _device(st.s, None, 10, 3, flags=True, stream=side, q_t=q_t)   # (no synchronisation in between)
    _same_topk(got, st.m_topk(st.queries * np.float32(2.0), 10, 3), "queries written on the stream")


# ---- 11. a batch of the headline's kind, small ---------------------------------------------------------------------------
def test_batch_of_the_headline_kind(pqv):
    st = Setup(pqv, 20000, 768, 64, "normal", 11000, nq=1024)
    got = _device(st.s, st.queries, 10, 8)
    pick = np.arange(0, 1024, 32)
    exp = st.m_topk(st.queries[pick], 10, 8)
    _same_topk(tuple(x[pick] for x in got[:4]), exp, "32 of 1024 queries")
    assert (got[2] == 10).all()
    host = st.s.topk(st.queries, 10, 8, metric=pqv.PQV_DOT)
    for x, y in zip(host, got[:4]):
        assert (np.asarray(x).view(np.uint8) == np.asarray(y).view(np.uint8)).all()      # host form == device form
