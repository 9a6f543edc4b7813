"""The screened centroid probe of a batch (probe_screen_kernel + probe_resolve_kernel; option probe_screen) against the exact one
(probe_rows_kernel; probe_screen = 0) and against the oracle: rows, distance BITS, n_found and n_candidates of topk / topk_device,
of topk under a candidate cap in the middle of a probed list (the cap cuts the concatenation in probe ORDER), and of a range
search.  Shapes: centroid counts off the 64- and 256-centroid tiles, dims off the 64-value K stage, batches off the 64-query
tile, nprobe 1 .. n_clusters (beyond n_clusters / 4 the plan keeps the exact kernel).  Data: uniform, tied centroids, queries
that ARE centroids, hostile offsets and scales, non-finite queries.  Rows wider than one 768-dim slab of the resolve, batches at the
edges of the 64-query tile, tables beyond what the resolve parks in LDS and beyond its contender cap (tests/probe_screen_cases.py,
held to their premises by tests/test_probe_screen_bound.py); the rule at the DEFAULT option, and tables the screen must refuse."""
import re

import numpy as np
import pytest

import probe_screen_cases as psc

pytestmark = pytest.mark.gpu

_CASES = {}
SCREENED = "probe_screen_kernel + probe_resolve_kernel"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assign(data, cent):
    """any assignment makes a valid index: the nearest centroid in f64"""
    with np.errstate(invalid="ignore"):          # (a centroid with an inf component: inf - inf)
        d = (data.astype(np.float64) ** 2).sum(1)[:, None] - 2.0 * data.astype(np.float64) @ cent.astype(np.float64).T \
            + (cent.astype(np.float64) ** 2).sum(1)[None, :]
        a = np.argmin(np.nan_to_num(d, nan=np.inf, posinf=np.inf), axis=1)
    return [np.flatnonzero(a == c).astype(np.uint32) for c in range(len(cent))]


def _data(kind, kc, dim, rng):
    n = max(3 * kc, 600)
    if kind == "uniform":
        data = rng.random((n, dim), dtype=np.float32)
    elif kind == "offset":
        data = (np.float32(-1000) + np.float32(0.01) * rng.standard_normal((n, dim))).astype(np.float32)
    elif kind == "scaled":
        data = (rng.random((n, dim), dtype=np.float32) * np.float32(1e-3)).astype(np.float32)
    elif kind == "outlier":
        data = rng.random((n, dim), dtype=np.float32)
    elif kind == "huge":
        # next to FLT_MAX: |c - mean|^2 in (1.9e38, 2.9e38), the centroids in +- pairs (their mean is exactly zero), rows and
        # queries on top of them -- finite norms whose sums overflow inside the bound
        big = np.sqrt(2.4e38 / dim)
        sgn = np.where(rng.random((kc // 2, dim)) < 0.85, 1.0, -1.0)
        half = (big * (0.9 + 0.2 * rng.random((kc // 2, 1))) * sgn).astype(np.float32)
        half[3] = np.float32(0.6) * half[2]
        cent = np.concatenate([half, -half])
        data = (cent[rng.integers(0, kc, n)] * (1.0 + 1e-3 * rng.standard_normal((n, 1)))).astype(np.float32)
        return data, cent
    else:
        raise ValueError(kind)
    cent = data[rng.choice(n, kc, replace=False)].copy()
    if kind == "outlier":
        cent[kc // 2] = np.float32(1e15)
    return data, cent


def _case(oracle, kind, kc, dim, table=None):
    key = (kind, kc, dim)
    if key not in _CASES:
        rng = np.random.default_rng(kc * 1000 + dim + len(kind))
        if table is not None:
            data, cent = table
            assert cent.shape == (kc, dim)
            oidx = oracle.index_from_parts(dim, cent, _assign(data, cent))
        elif kind == "tied":
            # 40 distinct points, many copies, 64 clusters: k-means leaves empty clusters at zero and duplicate centroids
            pts = rng.random((40, dim), dtype=np.float32)
            data = np.repeat(pts, 20, axis=0)
            oidx = oracle.build_index(data, n_clusters=64, workers=1, max_iters=3)
        else:
            data, cent = _data(kind, kc, dim, rng)
            oidx = oracle.index_from_parts(dim, cent, _assign(data, cent))
        _CASES[key] = (data, oidx)
    return _CASES[key]


def _searchers(pqv, data, oidx):
    blob = oidx.to_bytes()
    s2 = pqv.Searcher(pqv.Index.from_bytes(blob), pqv.Corpus.upload(data))
    s0 = pqv.Searcher(pqv.Index.from_bytes(blob), pqv.Corpus.upload(data))
    s2.set_option("probe_screen", 2)
    s0.set_option("probe_screen", 0)
    return s2, s0


def _queries(data, oidx, nq, rng, kind):
    dim = data.shape[1]
    q = data[rng.choice(len(data), nq)] + (np.float32(1e-3) * rng.standard_normal((nq, dim)).astype(np.float32)) * np.abs(data).mean()
    q = q.astype(np.float32)
    cent = oidx.centroids
    q[0] = cent[0]                                  # queries that ARE centroids
    q[nq - 1] = cent[len(cent) - 1]
    if kind == "uniform" and nq > 4:
        q[2] = q[2] * np.float32(1e6)               # far outside the data
    return q


def _same(a, b, what, found_only=False):
    if found_only:          # the oracle pads the slots beyond n_found its own way
        assert np.array_equal(a[2], b[2]), (what, "n_found")
        live = np.arange(a[0].shape[1])[None, :] < np.asarray(a[2])[:, None]
        a = (np.where(live, a[0], 0), np.where(live, a[1], 0), a[2], a[3])
        b = (np.where(live, b[0], 0), np.where(live, b[1], 0), b[2], b[3])
    for x, y, name in zip(a, b, ("rows", "dist", "n_found", "n_candidates")):
        if name == "dist":
            assert np.array_equal(_bits(x), _bits(y)), (what, name)
        else:
            assert np.array_equal(x, y), (what, name)


def _nprobes(kc):
    return [1, 7, kc // 4, kc // 4 + 1, kc]


def _check_case(pqv, oracle, kind, kc, dim, nq, with_oracle=True, table=None, queries=None, nprobes=None, refused=False):
    """table: (data, centroids) of a hand-made case `kind` (else _case makes it); queries: the batch (else _queries);
    nprobes: the depths (else _nprobes(kc)); refused: a table the screen cannot hold -- option 2 keeps the exact kernel"""
    import torch
    data, oidx = _case(oracle, kind, kc, dim, table)
    kc = oidx.n_clusters
    s2, s0 = _searchers(pqv, data, oidx)
    rng = np.random.default_rng(nq + dim)
    if queries is None:
        queries = _queries(data, oidx, nq, rng, kind)
    assert queries.shape == (nq, dim)
    k = 5
    for nprobe in (_nprobes(kc) if nprobes is None else nprobes):
        d2, d0 = s2.describe(nq, k, nprobe), s0.describe(nq, k, nprobe)
        assert SCREENED not in d0
        assert (SCREENED in d2) == (nprobe <= kc // 4 and dim % 4 == 0 and not refused), (nprobe, d2)       # beyond kc / 4: the exact kernel
        assert not refused or "centroid probe: probe_rows_kernel" in d2, d2
        got, ref = s2.topk(queries, k, nprobe), s0.topk(queries, k, nprobe)
        _same(got, ref, (kind, nprobe))
        if with_oracle:
            _same(got, oidx.topk_batch(data, queries, k, nprobe), (kind, nprobe, "oracle"), found_only=True)
        if nprobe == 7:
            # the probe ORDER: a cap in the middle of a probed list
            cap = int(got[3].min()) // 2 + 1
            got_c = s2.topk(queries, k, nprobe, max_candidates=cap)
            _same(got_c, s0.topk(queries, k, nprobe, max_candidates=cap), (kind, "cap"))
            if with_oracle:
                for q in range(0, nq, max(1, nq // 4)):
                    want = oidx.find_closest_centroids(queries[q], nprobe)
                    cand = oidx.candidate_rows(queries[q], nprobe)
                    lists = oidx.lists()
                    assert np.array_equal(cand, np.concatenate([lists[int(c)] for c in want]))
                    cand = cand[:cap]
                    dd = np.array([oracle.l2_ref4(queries[q], data[r]) for r in cand], np.float32)
                    order = np.lexsort((np.arange(len(cand)), dd.view(np.uint32)))[:k]
                    assert (_bits(got_c[1][q, :len(order)]) == _bits(np.sqrt(dd[order]))).all(), (kind, q)
            # one range search: half of the candidates of query 1 within the radius
            radius = float(np.sort(np.sqrt(np.array([oracle.l2_ref4(queries[1], data[r]) for r in oidx.candidate_rows(queries[1], nprobe)], np.float32)))[3])
            r2, r0 = s2.range_search(queries, radius, nprobe), s0.range_search(queries, radius, nprobe)
            for x, y in zip(r2, r0):
                assert np.array_equal(_bits(x) if x.dtype == np.float32 else x, _bits(y) if y.dtype == np.float32 else y), (kind, "range")
            # the device form
            dq = torch.from_numpy(queries).cuda()
            outs = []
            for s in (s2, s0):
                rows = torch.zeros((nq, k), dtype=torch.int32, device="cuda")
                dist = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
                nf = torch.zeros(nq, dtype=torch.int32, device="cuda")
                nc = torch.zeros(nq, dtype=torch.int64, device="cuda")
                st = torch.cuda.current_stream().cuda_stream
                s.topk_device(dq.data_ptr(), nq, k, nprobe, rows.data_ptr(), dist.data_ptr(), nf.data_ptr(), nc.data_ptr(), stream=st or 1)
                torch.cuda.synchronize()
                outs.append((rows.cpu().numpy().view(np.uint32), dist.cpu().numpy(), nf.cpu().numpy().view(np.uint32), nc.cpu().numpy().view(np.uint64)))
            _same(outs[0], outs[1], (kind, "device"))
    s2.close()
    s0.close()


def _stats(err, n_lines=2):
    """the counter lines the freed searchers printed -> (queries, exact evaluations per query, all-exact queries) of the one that
    screened (the option-0 searcher prints a line of zeros)"""
    m = [re.search(r"screened probe: (\d+) queries, ([0-9.]+) exact evaluations per query of (\d+) centroids, (\d+) all-exact", l) for l in err.splitlines()]
    m = [x for x in m if x]
    assert len(m) == n_lines, err
    ran = max(m, key=lambda x: int(x.group(1)))
    return int(ran.group(1)), float(ran.group(2)), int(ran.group(4))


def _uniform_with_stats(pqv, oracle, monkeypatch, capfd, kc, dim, nq):
    monkeypatch.setenv("PQV_PROBE_SCREEN_STATS", "1")
    capfd.readouterr()
    _check_case(pqv, oracle, "uniform", kc, dim, nq)
    err = capfd.readouterr().err
    n_queries, per_query, n_allexact = _stats(err)
    assert n_queries >= 3 * nq                                  # nprobe 1, 7 and kc / 4, at least one call each
    n_calls = n_queries // nq
    assert n_allexact <= (n_calls if nq > 4 else 0), err        # at most the far-out query of every call
    assert per_query < kc                                       # ... so the screen did exclude centroids


@pytest.mark.parametrize("kc,dim,nq", [(65, 4, 8), (130, 36, 17), (1000, 100, 100), (130, 768, 100), (1000, 768, 17), (65, 100, 100)])
def test_screened_probe_uniform(pqv, oracle, monkeypatch, capfd, kc, dim, nq):
    """Uniform data, every shape; the diagnostic counter (PQV_PROBE_SCREEN_STATS, printed when a searcher is freed) shows that the
    screen ran and that no query but the one placed 10^6 x outside the data took the all-exact fallback."""
    _uniform_with_stats(pqv, oracle, monkeypatch, capfd, kc, dim, nq)


# PR_GS = 192 float4 groups: a row of more than 768 dims takes probe_resolve_kernel's slab loop round again (the running sum carried
# over, the G - gs0 tail, the clamped reads of the last slab), probe_screen_kernel more than 12 K stages per tile; beyond 2048 dims
# (or with dim % 8 != 0) center_normalize_f16_kernel leaves its register path and the bound's constants count its other depth.
@pytest.mark.parametrize("kc,dim,nq", [
    (65, 772, 17),            # one group in the second slab, dim_p 832: 13 K stages
    (130, 1536, 65),          # two full slabs; one live row in the second query tile
    (65, 2048, 17),           # the last dim of the normalise kernel's register path
    (65, 2052, 8),            # its other path, dim % 8 != 0, three slabs
    (65, 3072, 17),           # four slabs
])
def test_screened_probe_wide_rows(pqv, oracle, monkeypatch, capfd, kc, dim, nq):
    _uniform_with_stats(pqv, oracle, monkeypatch, capfd, kc, dim, nq)


@pytest.mark.parametrize("nq", [64, 65, 129])
def test_screened_probe_batch_edges(pqv, oracle, monkeypatch, capfd, nq):
    """A full 64-query tile, a second tile with ONE live row (the others clamped to it), a third tile."""
    _uniform_with_stats(pqv, oracle, monkeypatch, capfd, 130, 36, nq)


def test_screened_probe_large_table(pqv, oracle, monkeypatch, capfd):
    """3201 centroids: above 3136 the bounds no longer fit probe_resolve_kernel's LDS and every read makes them again; kc_pad 3328
    leaves 127 padded centroids."""
    _uniform_with_stats(pqv, oracle, monkeypatch, capfd, 3201, 8, 17)


@pytest.mark.parametrize("kc", psc.ALL_EQUAL_KC)
def test_screened_probe_all_equal_table(pqv, oracle, monkeypatch, capfd, kc):
    """Every centroid the same point, more of them than PR_CAP = 2048: every centroid is a contender of every query
    (tests/test_probe_screen_bound.py holds the table to that), the `slot < PR_CAP` guard drops what the list cannot hold and the
    query evaluates EVERY centroid -- with the bounds parked in LDS (2304) and made again per read (3328).  The merge's
    (distance, index) order decides among kc equal distances."""
    data, cent, queries = psc.all_equal(kc)
    monkeypatch.setenv("PQV_PROBE_SCREEN_STATS", "1")
    capfd.readouterr()
    _check_case(pqv, oracle, "all_equal", kc, psc.DIM, psc.NQ, table=(data, cent), queries=queries)
    err = capfd.readouterr().err
    n_queries, per_query, n_allexact = _stats(err)
    assert n_queries >= 3 * psc.NQ and n_queries % psc.NQ == 0, err
    assert n_allexact == n_queries and per_query == kc, err


def test_screened_probe_2040_contenders(pqv, oracle, monkeypatch, capfd):
    """2040 copies of one point and 264 far centroids, queries beside the copies: 2040 contenders each, 64 rounds of 32 below the
    cap -- nobody goes all-exact at nprobe 1 and 7, not the query placed beside a far centroid either, which keeps a handful
    (tests/test_probe_screen_bound.py: 2040 for every query but that one)."""
    data, cent, queries = psc.split_2040()
    kc, nq = len(cent), psc.NQ
    monkeypatch.setenv("PQV_PROBE_SCREEN_STATS", "1")
    _, oidx = _case(oracle, "split_2040", kc, psc.DIM, (data, cent))
    for nprobe in (1, 7):
        # ONE call on a pair of its own: the counters of exactly nq queries
        capfd.readouterr()
        s2, s0 = _searchers(pqv, data, oidx)
        assert SCREENED in s2.describe(nq, 5, nprobe)
        _same(s2.topk(queries, 5, nprobe), s0.topk(queries, 5, nprobe), ("split_2040", nprobe, "one call"))
        s2.close()
        s0.close()
        err = capfd.readouterr().err
        n_queries, per_query, n_allexact = _stats(err)
        assert n_queries == nq and n_allexact == 0, err
        assert per_query >= psc.N_COPIES * (nq - 1) / nq, err
        # the copies are contenders of the nq - 1 near queries and of no one else; the far query keeps at least its nprobe nearest
        # and at most psc.FAR_MAX (per_query is printed to 0.01: nq * 0.005 < 0.5)
        far = round(per_query * nq) - psc.N_COPIES * (nq - 1)
        assert nprobe <= far <= psc.FAR_MAX[nprobe], (nprobe, far, err)
    # every output at every depth (from nprobe 576 on the far query is above the cap: all-exact)
    capfd.readouterr()
    _check_case(pqv, oracle, "split_2040", kc, psc.DIM, nq, table=(data, cent), queries=queries)
    n_queries, per_query, n_allexact = _stats(capfd.readouterr().err)
    assert n_queries >= 3 * nq and 0 < n_allexact < n_queries


# ---- the rule: the option at its default ---------------------------------------------------------------------------------------------
def _default_searcher(pqv, data, oidx):
    return pqv.Searcher(pqv.Index.from_bytes(oidx.to_bytes()), pqv.Corpus.upload(data))


def test_the_rule_under_the_default_option(pqv, oracle, monkeypatch):
    """No set_option call, no PQV_PROBE_SCREEN: the route users get (pqv.h: >= 128 queries, >= 256 centroids, nprobe <=
    n_clusters / 4, no table, not PQV_DOT -- and only where the batched probe runs at all: dim % 4 == 0)."""
    from pq_vector_amd import _ffi
    monkeypatch.delenv("PQV_PROBE_SCREEN", raising=False)
    data, oidx = _case(oracle, "uniform", 256, 8)
    s = _default_searcher(pqv, data, oidx)
    for nprobe in (1, 7, 64):
        assert SCREENED in s.describe(128, 5, nprobe), nprobe
        assert SCREENED in s.describe(129, 5, nprobe) and SCREENED in s.describe(1024, 5, nprobe), nprobe
        assert SCREENED not in s.describe(127, 5, nprobe), nprobe
        assert SCREENED not in s.describe(128, 5, nprobe, _ffi.PQV_DOT), nprobe
    assert SCREENED not in s.describe(128, 5, 65) and SCREENED not in s.describe(128, 5, 256)
    # one call of each kind at the default against the option-0 searcher, bit for bit
    s0 = _default_searcher(pqv, data, oidx)
    s0.set_option("probe_screen", 0)
    assert SCREENED not in s0.describe(128, 5, 7)
    queries = _queries(data, oidx, 128, np.random.default_rng(128), "uniform")
    _same(s.topk(queries, 5, 7), s0.topk(queries, 5, 7), "default topk")
    _same(s.topk(queries, 5, 7), oidx.topk_batch(data, queries, 5, 7), "default topk, oracle", found_only=True)
    radius = float(np.sqrt(np.float32(oracle.l2_ref4(queries[1], data[int(oidx.candidate_rows(queries[1], 7)[2])]))))
    for x, y in zip(s.range_search(queries, radius, 7), s0.range_search(queries, radius, 7)):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), "default range"
    s.close()
    s0.close()

    data, oidx = _case(oracle, "uniform", 255, 8)
    s = _default_searcher(pqv, data, oidx)
    for nprobe in (1, 7, 63):
        assert SCREENED not in s.describe(128, 5, nprobe) and SCREENED not in s.describe(1024, 5, nprobe), nprobe
    s.set_option("probe_screen", 2)               # (the kernels do support it: the rule kept it away)
    assert SCREENED in s.describe(128, 5, 7)
    s.close()


def test_never_screened_for_odd_dims_or_tables(pqv, oracle, monkeypatch):
    """dim % 4 != 0 has no batched probe to screen, a table probes per file: not at option 2 either."""
    monkeypatch.delenv("PQV_PROBE_SCREEN", raising=False)
    data, oidx = _case(oracle, "uniform", 256, 6)
    s = _default_searcher(pqv, data, oidx)
    s.set_option("probe_screen", 2)
    for nq, nprobe in ((128, 1), (128, 7), (128, 64), (8, 7)):
        assert SCREENED not in s.describe(nq, 5, nprobe), (nq, nprobe)
    s.close()
    data, oidx = _case(oracle, "uniform", 256, 8)
    corpus = pqv.Corpus.upload(data)
    t = pqv.TableSearcher([pqv.Index.from_bytes(oidx.to_bytes())], corpus, [0])
    t.set_option("probe_screen", 2)
    for nq, nprobe in ((128, 1), (128, 7), (128, 64), (8, 7)):
        assert SCREENED not in t.describe(nq, 5, nprobe), (nq, nprobe)
    t.close()
    corpus.close()


@pytest.mark.parametrize("name", ["norm above 3e38", "inf component"])
def test_screened_probe_refuses_the_table(pqv, oracle, name):
    """A centroid whose |c - mean|^2 exceeds 3e38 (every component finite), a centroid with an inf component: the images are not
    made, option 2 keeps probe_rows_kernel, the answers are option 0's."""
    data, cent = psc.refused_tables()[name]
    kc, dim = cent.shape
    queries = (data[np.random.default_rng(9).choice(len(data), 17)] * np.float32(1.0005)).astype(np.float32)
    _check_case(pqv, oracle, name, kc, dim, 17, with_oracle=False, table=(data, cent), queries=queries, refused=True)


def test_screened_probe_tied_centroids(pqv, oracle, monkeypatch, capfd):
    """40 distinct points and 64 clusters: empty clusters stay at zero and duplicate centroids tie, also at the P-th place --
    every tied centroid stays a contender, the merge's (distance, index) order decides as before; no fallback."""
    monkeypatch.setenv("PQV_PROBE_SCREEN_STATS", "1")
    capfd.readouterr()
    _check_case(pqv, oracle, "tied", 64, 36, 17)
    err = capfd.readouterr().err
    m = [x for x in (re.search(r"screened probe: (\d+) queries, .* (\d+) all-exact", l) for l in err.splitlines()) if x]
    assert len(m) == 2 and max(int(x.group(1)) for x in m) >= 3 * 17, err
    assert all(int(x.group(2)) == 0 for x in m), err


@pytest.mark.parametrize("kind", ["offset", "scaled", "outlier", "huge"])
def test_screened_probe_hostile_data(pqv, oracle, kind):
    """Data at -1000 +- 0.01, data scaled by 10^-3, one centroid at 10^15, norms next to FLT_MAX (sums inside the bound overflow:
    such a pair must stay a contender, never get a made-up bound): the bound may be loose (a query may evaluate every
    centroid), the answer may not differ."""
    _check_case(pqv, oracle, kind, 130, 36, 17)


def test_screened_probe_nonfinite_queries(pqv, oracle):
    """A query with a NaN and one with an Inf: whatever the exact probe answers."""
    data, oidx = _case(oracle, "uniform", 130, 36)
    s2, s0 = _searchers(pqv, data, oidx)
    rng = np.random.default_rng(3)
    queries = rng.random((17, 36), dtype=np.float32)
    queries[3, 5] = np.nan
    queries[9, 0] = np.inf
    queries[12, 35] = -np.inf
    for nprobe in (1, 7, 32):
        assert SCREENED in s2.describe(17, 5, nprobe)
        _same(s2.topk(queries, 5, nprobe), s0.topk(queries, 5, nprobe), nprobe)
        _same(s2.topk(queries, 5, nprobe, max_candidates=40), s0.topk(queries, 5, nprobe, max_candidates=40), (nprobe, "cap"))


def test_option_after_creation_without_images(pqv, oracle, monkeypatch):
    """A searcher created under PQV_PROBE_SCREEN=0 has no centroid images; the first non-zero set_option makes them."""
    data, oidx = _case(oracle, "uniform", 130, 36)
    monkeypatch.setenv("PQV_PROBE_SCREEN", "0")
    s = pqv.Searcher(pqv.Index.from_bytes(oidx.to_bytes()), pqv.Corpus.upload(data))
    monkeypatch.delenv("PQV_PROBE_SCREEN")
    queries = np.random.default_rng(5).random((17, 36), dtype=np.float32)
    assert SCREENED not in s.describe(17, 5, 7)
    ref = s.topk(queries, 5, 7)
    s.set_option("probe_screen", 2)
    assert SCREENED in s.describe(17, 5, 7)
    _same(s.topk(queries, 5, 7), ref, "lazy images")
