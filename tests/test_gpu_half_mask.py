"""Row-masked search over f16 corpora (pqv.h: half-precision corpora, "masked") on both routes -- masked_stream_h_kernel, and under
rerank_mode 2 the screened route -- against the f32 masked calls of a Searcher over the widened rows under the same allow bytes: row ids,
distance BITS, n_found, n_candidates, lims and n_within equal, no tolerance.  Index as in test_gpu_half_screen.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REF4, SEQ, N, KC, KMAX = 0, 1, 3000, 12, 127
CUTS = [0, 1, 1, 1301] + list(np.linspace(1301, N, KC - 2).astype(int)[1:])      # list 0 one row, list 1 empty, list 2 positions [1, 1301)
MASKS = ["half", "sparse", "ones", "zeros", "block", "km1"]
COUNTED = ("queries", "candidate_rows", "embeddings_fetched")
_CASE, _MASK = {}, {}


def _case(pqv, oracle, dim, hostile=0):
    """(row of every list position, [default f16 searcher, screened f16 searcher, f32 searcher over the widened rows], 70 queries)"""
    if (dim, hostile) not in _CASE:
        rng = np.random.default_rng(2000 + dim + (7 if hostile else 0))
        if hostile:       # small integers: many equal distances; 2: a few rows with Inf / NaN halves
            h = rng.integers(0, 3, size=(N, dim)).astype(np.float16)
            if hostile == 2:
                h[rng.choice(N, size=6, replace=False), 0] = np.array([np.inf, -np.inf, np.nan, np.inf, np.nan, -np.inf], dtype=np.float16)
        else:
            h = rng.standard_normal((N, dim)).astype(np.float16)
        wide = h.astype(np.float32)
        cents = oracle.build_index(np.clip(np.nan_to_num(wide, posinf=4, neginf=-4), -4, 4), n_clusters=KC, workers=4).centroids
        order = np.argsort(rng.integers(0, KC, size=N), kind="stable").astype(np.uint32)
        index = pqv.Index.from_parts(dim, cents, [order[CUTS[i]:CUTS[i + 1]] for i in range(KC)])
        sh, s2 = pqv.Searcher(index, pqv.Corpus.upload(h)), pqv.Searcher(index, pqv.Corpus.upload(h)).set_option("rerank_mode", 2)
        queries = np.random.default_rng(6007 + dim).standard_normal((70, dim)).astype(np.float32)
        _CASE[(dim, hostile)] = (order, [sh, s2, pqv.Searcher(index, pqv.Corpus.upload(wide))], queries)
    return _CASE[(dim, hostile)]


def _masks(case_key, order, searchers, name, k=10):
    """the three searchers' RowMasks over the same allow bytes; positions are list order, position p reports row order[p]"""
    key = case_key + (name, k if name == "km1" else 0)
    if key not in _MASK:
        rng, p = np.random.default_rng(77), np.arange(N)
        pos = {"half": rng.random(N) < 0.5, "sparse": rng.random(N) < 0.02, "ones": p >= 0, "zeros": p < 0,
               "block": ((p // 64) % 3 != 0) & ((p < 1 + 1024) | (p >= 1301)),      # every third 64-position word, and list 2's whole second segment
               "km1": np.isin(p, rng.choice(N, size=k - 1, replace=False))}[name]     # k - 1 rows in all: with every list probed, each query finds exactly those
        allowed = pos[np.argsort(order)].astype(np.uint8)       # allowed[order[p]] = pos[p]
        _MASK[key] = [s.row_mask(allowed) for s in searchers]
    return _MASK[key]


def _same(got, exp):
    assert (got[2] == exp[2]).all() and (got[3] == exp[3]).all(), "n_found / n_candidates"
    assert (got[0] == exp[0]).all() and (got[1].view(np.uint32) == exp[1].view(np.uint32)).all(), "rows / distance bits"


def _device(s, mask, queries, k, nprobe, flags, **kw):
    import torch
    q, nq = torch.from_numpy(queries).cuda(), len(queries)
    rows, dist = torch.zeros((nq, k), dtype=torch.int32, device="cuda"), torch.zeros((nq, k), dtype=torch.float32, device="cuda")
    nf, nc, tie = (torch.zeros(nq, dtype=t, device="cuda") for t in (torch.int32, torch.int64, torch.int32))
    s.topk_device_f16(q.data_ptr(), nq, k, nprobe, rows.data_ptr(), dist.data_ptr(), nf.data_ptr(), nc.data_ptr(), mask=mask,
                      d_tie_flags=tie.data_ptr() if flags else 0, **kw)
    torch.cuda.synchronize()
    return (rows.cpu().numpy().view(np.uint32), dist.cpu().numpy(), nf.cpu().numpy().view(np.uint32), nc.cpu().numpy().view(np.uint64)), tie.cpu().numpy()


def _delta(s, c0, *names):
    return [s.counters()[n] - c0[n] for n in names]


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("dim", [8, 24, 30, 72, 264, 768])
def test_mask_dims(pqv, oracle, dim, mask):
    """every load form and chunk count, one and two query tiles on a list; dim 30 falls through to the exact route on both searchers"""
    order, (sh, s2, sf), queries = _case(pqv, oracle, dim)
    mh, m2, mf = _masks((dim, 0), order, (sh, s2, sf), mask)
    for nq in (1, 33, 70):
        q, c0 = queries[:nq], s2.counters()
        exp = sf.topk(q, 10, 5, mask=mf)
        _same(sh.topk_f16(q, 10, 5, mask=mh), exp)
        _same(s2.topk_f16(q, 10, 5, mask=m2), exp)
        pairs, surv = _delta(s2, c0, "screened_pairs", "screen_survivors")
        if mask in ("half", "block") and dim != 30:
            assert pairs > 0 and 0 < surv < pairs
        assert pairs == 0 or (dim != 30 and mask not in ("zeros", "km1")), "nothing to screen, or outside the route"
        assert mask != "zeros" or not exp[2].any()
        if mask == "ones":
            _same(exp, sh.topk(q, 10, 5))
    assert sh.counters()["screened_pairs"] == 0, "the default rerank_mode never screens"


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("k,nprobe,cap,sqrt_out", [(1, 5, 0, False), (10, 5, 0, False), (KMAX, 5, 0, False), (10, 64, 0, False), (10, 5, 1500, False),
                                                   (10, 5, 0, True)])
@pytest.mark.parametrize("dim", [24, 264])
def test_mask_parameters(pqv, oracle, dim, k, nprobe, cap, sqrt_out, mask):
    """each axis against the base case: host form and both device forms on both routes, and the counters a masked call advances"""
    order, (sh, s2, sf), queries = _case(pqv, oracle, dim)
    masks = _masks((dim, 0), order, (sh, s2, sf), mask, k)
    q, kw, c0 = queries[:33], dict(max_candidates=cap, sqrt_out=sqrt_out), sf.counters()
    exp, want = sf.topk(q, k, nprobe, mask=masks[2], **kw), _delta(sf, c0, *COUNTED)       # (left to right: the call, then what it counted)
    assert not (mask == "km1" and nprobe == 64) or (exp[2] == k - 1).all()
    for s, m in zip((sh, s2), masks):
        c0 = s.counters()
        _same(s.topk_f16(q, k, nprobe, mask=m, **kw), exp)
        assert _delta(s, c0, *COUNTED) == want
        got, tie = _device(s, m, q, k, nprobe, True, **kw)
        assert (tie == 0).all(), "continuous data must not tie (a condition on the inputs)"
        _same(got, exp)
        _same(_device(s, m, q, k, nprobe, False, **kw)[0], exp)


@pytest.mark.parametrize("mask", ["half", "sparse", "zeros", "block"])
@pytest.mark.parametrize("dim", [8, 24, 30, 72, 264, 768])
def test_mask_range(pqv, oracle, dim, mask):
    """range search (always the exact route) at the median allowed-candidate distance, and at inf cut to 7 results"""
    order, (sh, s2, sf), queries = _case(pqv, oracle, dim)
    masks, q = _masks((dim, 0), order, (sh, s2, sf), mask), queries[:33]
    every = sf.range_search(q, np.inf, 5, mask=masks[2], max_results=7)
    median = float(np.median(sf.range_search(q, np.inf, 5, mask=masks[2])[2])) if every[3].any() else 1.0
    near = sf.range_search(q, median, 5, mask=masks[2], max_candidates=1500)
    for s, m in zip((sh, s2), masks):
        for exp, got in ((every, s.range_search_f16(q, np.inf, 5, mask=m, max_results=7)), (near, s.range_search_f16(q, median, 5, mask=m, max_candidates=1500))):
            assert all((g.view(np.uint32) == e.view(np.uint32)).all() if g.dtype == np.float32 else (g == e).all() for g, e in zip(got, exp))


@pytest.mark.parametrize("hostile", [1, 2])
def test_mask_hostile(pqv, oracle, hostile):
    """equal distances, then Inf / NaN halves and non-finite queries: host form against the f32 call, screened flags against the exact route's"""
    order, (sh, s2, sf), queries = _case(pqv, oracle, 24, hostile)
    mh, m2, mf = _masks((24, hostile), order, (sh, s2, sf), "half")
    q = np.round(queries[:33]).astype(np.float32)
    if hostile == 2:
        q[5, 3], q[9, 0] = np.inf, np.nan
    exp = sf.topk(q, 10, 5, mask=mf)
    _same(sh.topk_f16(q, 10, 5, mask=mh), exp)
    _same(s2.topk_f16(q, 10, 5, mask=m2), exp)
    (got, tie), (ref, rtie) = _device(s2, m2, q, 10, 5, True), _device(sh, mh, q, 10, 5, True)
    keep = tie == 0
    assert tie.any() and (tie == rtie).all() and (got[2] == ref[2]).all()
    assert (got[0][keep] == ref[0][keep]).all() and (got[1][keep].view(np.uint32) == ref[1][keep].view(np.uint32)).all()


@pytest.mark.parametrize("dim,k,metric,flags", [(30, 10, REF4, True), (24, 10, SEQ, True), (24, KMAX + 1, REF4, True), (24, KMAX + 1, REF4, False)])
def test_mask_fall_through(pqv, oracle, dim, k, metric, flags):
    """outside the screened route's limits rerank_mode 2 changes nothing (k 128 is inside them without tie flags)"""
    order, (sh, s2, sf), queries = _case(pqv, oracle, dim)
    mh, m2, mf = _masks((dim, 0), order, (sh, s2, sf), "half")
    c0 = s2.counters()
    _same(_device(s2, m2, queries[:33], k, 5, flags, metric=metric)[0], _device(sh, mh, queries[:33], k, 5, flags, metric=metric)[0])
    assert (_delta(s2, c0, "screened_pairs")[0] > 0) == (k == KMAX + 1 and not flags)


def test_mask_refusals(pqv, oracle):
    """the _f16 forms need f16 rows, and refuse PQV_COSINE / PQV_DOT by the metric's name as the served f16 calls do"""
    order, (sh, s2, sf), queries = _case(pqv, oracle, 24)
    mh, m2, mf = _masks((24, 0), order, (sh, s2, sf), "half")
    refused = [(sf, mf, {}, "corpus rows are f32", pqv._ffi.PQV_ERR_INVALID)] + [(sh, mh, dict(metric=getattr(pqv, name)), name + " does not take f16 corpora", pqv._ffi.PQV_ERR_UNSUPPORTED) for name in ("PQV_COSINE", "PQV_DOT")]
    for call in (lambda s, m, **kw: s.topk_f16(queries[:4], 5, 3, mask=m, **kw), lambda s, m, **kw: s.range_search_f16(queries[:4], 1.0, 3, mask=m, **kw),
                 lambda s, m, **kw: _device(s, m, queries[:4], 5, 3, True, **kw)):
        for s, m, kw, text, code in refused:
            with pytest.raises(pqv.PqvError, match=text) as e:
                call(s, m, **kw)
            assert e.value.code == code
