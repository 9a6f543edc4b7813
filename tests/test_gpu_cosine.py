"""PQV_COSINE through the index on the GPU (include/pqv.h: PQV_COSINE).  Every cosine call is compared with the PQV_L2SQ_REF4
call (sqrt_out 0) of a REFERENCE SETUP -- a plain searcher over Index.from_parts(dim, n(centroids), lists) and a corpus of n(x),
queried with n(q), n the numpy restatement of tests/cosine_ref.py --: row ids, n_found, n_candidates, counters exactly, every
distance bit equal to 0.5f * d2.  Plus the CPU oracle over the normalised data, ties, tables, scale invariance, zero vectors,
no interference with L2, PQV_PREPARE_COSINE, agreement with pqv_brute_topk at nprobe = n_clusters and the C3 shape."""
import gc
import math

import numpy as np
import pytest

from cosine_ref import half, normalise, normalised_index
from range_oracle import l2_chain, REF4
from test_gpu_table import Table

pytestmark = pytest.mark.gpu

_DATA = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _mixture(rng, n, dim, kc):
    centres = rng.standard_normal((kc, dim)).astype(np.float32)
    return (centres[rng.integers(0, kc, n)] + np.float32(0.3) * rng.standard_normal((n, dim)).astype(np.float32)).astype(np.float32)


def _case(oracle, n, dim, kc, kind, seed):
    key = (n, dim, kc, kind, seed)
    if key not in _DATA:
        rng = np.random.default_rng(seed)
        if kind == "mixture":
            data, q = _mixture(rng, n, dim, kc), _mixture(rng, 64, dim, kc)
        else:
            data, q = rng.random((n, dim), dtype=np.float32), rng.random((64, dim), dtype=np.float32)
        _DATA[key] = (data, q, oracle.build_index(data, n_clusters=kc, max_iters=5, workers=1))
    return _DATA[key]


class Pair:
    """The searcher under test (raw index and rows) and the reference setup (normalised ones), same flags."""

    def __init__(self, pqv, data, oidx, flags=0):
        dim = data.shape[1]
        self.data, self.oidx = data, oidx
        self.s = pqv.Searcher(pqv.Index.from_bytes(oidx.to_bytes()), pqv.Corpus.upload(data), flags)
        self.ndata = normalise(data)
        self.ref = pqv.Searcher(normalised_index(pqv, dim, oidx.centroids, oidx.lists()), pqv.Corpus.upload(self.ndata),
                                flags & ~pqv.PQV_PREPARE_COSINE)

    def set_option(self, name, value):
        self.s.set_option(name, value)
        self.ref.set_option(name, value)


def _check_topk(pqv, p, q, k, nprobe, max_candidates=0):
    got = p.s.topk(q, k, nprobe, max_candidates=max_candidates, metric=pqv.PQV_COSINE, sqrt_out=True)   # (sqrt_out ignored)
    exp = p.ref.topk(normalise(q), k, nprobe, max_candidates=max_candidates, metric=pqv.PQV_L2SQ_REF4, sqrt_out=False)
    _same_topk(got, exp)
    return got


def _same_topk(got, exp):
    rows, dist, nf, nc = got
    erows, edist, enf, enc = exp
    assert (nf == enf).all(), "n_found"
    assert (nc == enc).all(), "n_candidates"
    assert (rows == erows).all(), "row ids"
    assert (_bits(dist) == _bits(half(edist))).all(), "distance bits"


def _device(torch, s, metric, q, k, nprobe, max_candidates=0, flags=False, stream=None):
    dev = torch.device("cuda", 0)
    q_t = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(dev)
    nq = len(q)
    r_t = torch.full((nq, k), -1, dtype=torch.int32, device=dev)
    d_t = torch.full((nq, k), float("inf"), dtype=torch.float32, device=dev)
    nf_t = torch.zeros(nq, dtype=torch.int32, device=dev)
    nc_t = torch.zeros(nq, dtype=torch.int64, device=dev)
    tf_t = torch.full((nq,), 7, dtype=torch.int32, device=dev)
    st = stream if stream is not None else torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        s.topk_device(q_t.data_ptr(), nq, k, nprobe, r_t.data_ptr(), d_t.data_ptr(), nf_t.data_ptr(), nc_t.data_ptr(),
                      max_candidates=max_candidates, metric=metric, sqrt_out=False, stream=st.cuda_stream,
                      d_tie_flags=tf_t.data_ptr() if flags else 0)
    st.synchronize()
    return (r_t.cpu().numpy().view(np.uint32), d_t.cpu().numpy(), nf_t.cpu().numpy().astype(np.uint32),
            nc_t.cpu().numpy().astype(np.uint64), tf_t.cpu().numpy())


def _check_device(pqv, torch, s, ref, q, k, nprobe, max_candidates=0):
    for flags in (False, True):
        got = _device(torch, s, pqv.PQV_COSINE, q, k, nprobe, max_candidates, flags)
        exp = _device(torch, ref, pqv.PQV_L2SQ_REF4, normalise(q), k, nprobe, max_candidates, flags)
        _same_topk(got[:4], exp[:4])
        assert (got[4] == exp[4]).all(), "tie flags"


def _check_range(pqv, s, ref, q, nprobe, radius, max_candidates=0, max_results=0):
    got = s.range_search(q, radius, nprobe, max_candidates=max_candidates, max_results=max_results, metric=pqv.PQV_COSINE)
    exp = ref.range_search(normalise(q), 2.0 * radius, nprobe, max_candidates=max_candidates, max_results=max_results,
                           metric=pqv.PQV_L2SQ_REF4, sqrt_out=False)
    lims, rows, dist, nw, nc = got
    elims, erows, edist, enw, enc = exp
    assert (nc == enc).all() and (nw == enw).all() and (lims == elims).all() and (rows == erows).all()
    assert (_bits(dist) == _bits(half(edist))).all()
    assert (dist <= np.float32(radius)).all()
    return got


def _radius(pqv, s, ref, q, nprobe):
    """The 41st cosine distance of the first query (the same call on the reference setup: the counters stay in step)."""
    _, d, _, _ = s.topk(q[:1], 64, nprobe, metric=pqv.PQV_COSINE)
    ref.topk(normalise(q[:1]), 64, nprobe, sqrt_out=False)
    return float(d[0, 40])


@pytest.mark.parametrize("kind", ["uniform", "mixture"])
@pytest.mark.parametrize("dim", [3, 8, 30, 128, 768, 1536])
def test_cosine_equals_the_normalised_reference_setup(pqv, oracle, dim, kind):
    import torch
    n = {768: 3000, 1536: 4000}.get(dim, 4000)
    data, q, oidx = _case(oracle, n, dim, 12, kind, dim)
    p = Pair(pqv, data, oidx)
    k, nprobe = 10, 3
    _check_topk(pqv, p, q, k, nprobe)
    _check_topk(pqv, p, q[:1], k, nprobe)
    _check_topk(pqv, p, q, k, nprobe, max_candidates=500)
    _check_device(pqv, torch, p.s, p.ref, q, k, nprobe)
    _check_device(pqv, torch, p.s, p.ref, q[:1], k, nprobe)
    _check_device(pqv, torch, p.s, p.ref, q, k, nprobe, max_candidates=700)
    radius = _radius(pqv, p.s, p.ref, q, nprobe)
    got = _check_range(pqv, p.s, p.ref, q, nprobe, radius)
    assert got[0][-1] > 0
    _check_range(pqv, p.s, p.ref, q, nprobe, radius, max_results=5)
    _check_range(pqv, p.s, p.ref, q, nprobe, radius, max_candidates=300)
    # counters advance as the reference setup's
    assert p.s.counters() == p.ref.counters()


@pytest.mark.parametrize("layout", ["row", "release"])
def test_cosine_other_layouts(pqv, oracle, layout):
    import torch
    data, q, oidx = _case(oracle, 4000, 256, 12, "mixture", 11)
    flags = pqv.PQV_LAYOUT_ROW_ORDER if layout == "row" else pqv.PQV_RELEASE_ROW_ORDER
    p = Pair(pqv, data, oidx, flags)
    _check_topk(pqv, p, q, 10, 4)
    _check_device(pqv, torch, p.s, p.ref, q, 10, 4)
    _check_range(pqv, p.s, p.ref, q, 4, _radius(pqv, p.s, p.ref, q, 4))


@pytest.mark.parametrize("option,value", [("rerank_mode", 1), ("rerank_mode", 2), ("screen_i8", 0), ("tile_filter", 2),
                                          ("tile_filter", 0), ("wide_quads", 2)])
def test_cosine_forced_dispatch_paths(pqv, oracle, option, value):
    import torch
    data, q, oidx = _case(oracle, 6000, 768, 8, "uniform", 21)
    p = Pair(pqv, data, oidx)
    _check_topk(pqv, p, q[:2], 10, 2)             # the layout is built before the option: set_option must reach it
    p.set_option(option, value)
    qq = np.concatenate([q, q[::-1], q[:32]])      # 160 queries on 2 of 8 lists: the wide-quad sizes
    _check_topk(pqv, p, qq, 10, 2)
    _check_device(pqv, torch, p.s, p.ref, qq, 10, 2)
    _check_device(pqv, torch, p.s, p.ref, qq, 100, 2)
    assert p.s.describe(len(qq), 10, 2, pqv.PQV_COSINE).startswith("PQV_COSINE: normalize_rows_kernel")


def test_cosine_against_the_cpu_oracle(pqv, oracle):
    data, q, oidx = _case(oracle, 4000, 128, 12, "mixture", 31)
    dim = data.shape[1]
    p = Pair(pqv, data, oidx)
    rows, dist, nf, nc = p.s.topk(q, 10, 3, metric=pqv.PQV_COSINE)
    nidx = oracle.index_from_parts(dim, normalise(np.asarray(oidx.centroids).reshape(-1, dim)), oidx.lists())
    nq_ = normalise(q)
    orows, _, onf, onc = nidx.topk_batch(p.ndata, nq_, 10, 3)
    assert (rows == orows).all() and (nf == onf).all() and (nc == onc).all()
    for i in range(len(q)):
        d2 = l2_chain(p.ndata[rows[i, :nf[i]]], nq_[i], REF4)
        assert (_bits(dist[i, :nf[i]]) == _bits(half(d2))).all()


def test_cosine_ties_duplicates_and_zero_vectors(pqv, oracle):
    import torch
    rng = np.random.default_rng(41)
    data = rng.integers(0, 3, (3000, 16)).astype(np.float32)          # integer values: many exact ties, duplicate rows
    data[::97] = 0.0                                                  # zero rows
    oidx = oracle.build_index(data, n_clusters=10, max_iters=5, workers=1)
    p = Pair(pqv, data, oidx)
    q = rng.integers(0, 3, (40, 16)).astype(np.float32)
    q[0] = 0.0                                                        # a zero query: every row at 0.5 * sq(n(x))
    q[1] = data[5]
    rows, dist, nf, _ = _check_topk(pqv, p, q, 20, 4)
    assert p.s.counters()["exact_replays"] == p.ref.counters()["exact_replays"] > 0
    # (the probe ranks the NORMALISED centroids: the candidates are the normalised index' own)
    nidx = oracle.index_from_parts(16, normalise(np.asarray(oidx.centroids).reshape(-1, 16)), oidx.lists())
    cand = nidx.candidate_rows(np.zeros(16, np.float32), 4)
    assert (_bits(dist[0, :nf[0]]) == _bits(np.sort(half(l2_chain(p.ndata[cand], np.zeros(16, np.float32), REF4)))[:nf[0]])).all()
    _check_device(pqv, torch, p.s, p.ref, q, 20, 4)
    _check_range(pqv, p.s, p.ref, q, 4, 0.1)
    _check_range(pqv, p.s, p.ref, q, 4, 0.0)
    _check_range(pqv, p.s, p.ref, q, 4, math.inf, max_results=50)


def test_cosine_power_of_two_scaled_queries_give_identical_bits(pqv, oracle):
    import torch
    data, q, oidx = _case(oracle, 4000, 768, 12, "mixture", 51)
    p = Pair(pqv, data, oidx)
    a = p.s.topk(q, 10, 3, metric=pqv.PQV_COSINE)
    for scale in (2.0, 0.5, 64.0):
        b = p.s.topk(q * np.float32(scale), 10, 3, metric=pqv.PQV_COSINE)
        assert all((x == y).all() for x, y in zip(a[:1] + a[2:], b[:1] + b[2:])) and (_bits(a[1]) == _bits(b[1])).all()
        da = _device(torch, p.s, pqv.PQV_COSINE, q, 10, 3)
        db = _device(torch, p.s, pqv.PQV_COSINE, q * np.float32(scale), 10, 3)
        assert (da[0] == db[0]).all() and (_bits(da[1]) == _bits(db[1])).all()


@pytest.mark.parametrize("rr", [False, True])
def test_cosine_tables(pqv, oracle, rr):
    import torch
    rng = np.random.default_rng(61 + rr)
    dim = 128
    flags = pqv.PQV_TABLE_CAP_ROUND_ROBIN if rr else 0
    t = Table(pqv, oracle, rng, [1500, 900, 2100], [6, 4, 9], dim, flags=flags)
    ndata = normalise(t.data)
    ref = pqv.TableSearcher([normalised_index(pqv, dim, o.centroids, o.lists()) for o in t.oidx], pqv.Corpus.upload(ndata),
                            t.row_base, flags=flags)
    q = rng.random((30, dim), dtype=np.float32)
    caps = (0, 250, 1000) if rr else (0,)
    for m in caps:
        for nprobe in (1, 3, 20):
            got = t.s.topk(q, 10, nprobe, max_candidates=m, metric=pqv.PQV_COSINE)
            exp = ref.topk(normalise(q), 10, nprobe, max_candidates=m, metric=pqv.PQV_L2SQ_REF4, sqrt_out=False)
            _same_topk(got, exp)
            _check_device(pqv, torch, t.s, ref, q, 10, nprobe, m)
            _check_range(pqv, t.s, ref, q, nprobe, 0.2, max_candidates=m)
    assert t.s.counters() == ref.counters()
    assert "table of 3 files" in t.s.describe(30, 10, 3, pqv.PQV_COSINE)


def test_cosine_leaves_l2_alone(pqv, oracle):
    import torch
    data, q, oidx = _case(oracle, 4000, 768, 12, "uniform", 71)
    corpus = pqv.Corpus.upload(data)
    s = pqv.Searcher(pqv.Index.from_bytes(oidx.to_bytes()), corpus)
    l2 = s.topk(q, 10, 3)
    l2d = _device(torch, s, pqv.PQV_L2SQ_REF4, q, 10, 3)
    fp0 = s.footprint()
    assert s.footprint() == fp0                                       # L2 calls leave it where it is
    c1 = s.topk(q, 10, 3, metric=pqv.PQV_COSINE)                      # builds the cosine layout
    fp1 = s.footprint()
    col = data.size * 4
    assert fp1["row_order_bytes"] + fp1["ivf_rows_bytes"] >= fp0["row_order_bytes"] + fp0["ivf_rows_bytes"] + col
    assert fp1["blocked_bytes"] > fp0["blocked_bytes"]
    l2b = s.topk(q, 10, 3)
    assert all((x == y).all() for x, y in zip(l2b, l2)) and (_bits(l2b[1]) == _bits(l2[1])).all()
    l2db = _device(torch, s, pqv.PQV_L2SQ_REF4, q, 10, 3)
    assert all((x == y).all() for x, y in zip(l2db, l2d)) and (_bits(l2db[1]) == _bits(l2d[1])).all()
    # PQV_PREPARE_COSINE: the same answers, the layout built at creation
    sp = pqv.Searcher(pqv.Index.from_bytes(oidx.to_bytes()), pqv.Corpus.upload(data), pqv.PQV_PREPARE_COSINE)
    fpp = sp.footprint()
    assert fpp["row_order_bytes"] + fpp["ivf_rows_bytes"] >= 2 * col
    c2 = sp.topk(q, 10, 3, metric=pqv.PQV_COSINE)
    assert all((x == y).all() for x, y in zip(c1, c2)) and (_bits(c1[1]) == _bits(c2[1])).all()
    assert sp.footprint()["blocked_bytes"] == fpp["blocked_bytes"]
    # a table made with the flag too
    tp = pqv.TableSearcher([pqv.Index.from_bytes(oidx.to_bytes())], pqv.Corpus.upload(data), [0], flags=pqv.PQV_PREPARE_COSINE)
    c3 = tp.topk(q, 10, 3, metric=pqv.PQV_COSINE)
    assert all((x == y).all() for x, y in zip(c1, c3)) and (_bits(c1[1]) == _bits(c3[1])).all()


def test_cosine_agrees_with_brute_force_at_full_probe(pqv, oracle):
    data, q, oidx = _case(oracle, 4000, 128, 12, "uniform", 81)
    corpus = pqv.Corpus.upload(data)
    s = pqv.Searcher(pqv.Index.from_bytes(oidx.to_bytes()), corpus)
    rows, dist, nf, _ = s.topk(q, 10, 12, metric=pqv.PQV_COSINE)
    brows, bdist, bnf = corpus.brute_topk(q, 10, pqv.PQV_COSINE)
    assert (nf == 10).all() and (bnf == 10).all()
    assert np.allclose(dist, bdist, rtol=1e-4, atol=1e-6)
    same = sum(len(set(a.tolist()) & set(b.tolist())) for a, b in zip(rows, brows))
    assert same >= 0.98 * rows.size, same


@pytest.mark.timeout(1500)
def test_cosine_c3_full_size_mixture(pqv):
    """10 M x 768 mixture (BASELINE C3's shape, 1024 clusters, nprobe 32), 64 queries, against the normalised reference setup
    (its rows normalised on the device with the same float32 chain, in torch)."""
    import os
    import torch
    import bench
    n, dim, kc, nprobe, _ = bench.WORKLOADS["c3"]
    k, nq = 10, 64
    dev = torch.device("cuda", 0)
    x_t = bench.synth_mixture(torch, dev, 1234, n, dim, kc)
    q = bench.synth_mixture(torch, dev, 7, nq, dim, kc).cpu().numpy()
    torch.cuda.synchronize()
    corpus = pqv.Corpus.from_device_ptr(x_t.data_ptr(), n, dim, device=0, keepalive=x_t)
    index = pqv.IndexBuilder(corpus).n_clusters(kc).max_iters(20).seed(42).workers(os.cpu_count() or 1).build()
    s = pqv.Searcher(index, corpus)
    # n(x) in torch: the 4-grouped chain, then f64 sqrt / division rounded once to f32 (both correctly rounded)
    nx_t = torch.empty_like(x_t)
    for r0 in range(0, n, 1 << 20):
        xb = x_t[r0:r0 + (1 << 20)]
        sq = xb * xb
        t = ((sq[:, 0::4] + sq[:, 1::4]) + sq[:, 2::4]) + sq[:, 3::4]
        acc = torch.zeros(len(xb), dtype=torch.float32, device=dev)
        for g in range(t.shape[1]):
            acc = acc + t[:, g]
        rt = torch.where(acc == 0, torch.zeros_like(acc), (1.0 / torch.sqrt(acc.double()).float().double()).float())
        nx_t[r0:r0 + len(xb)] = xb * rt[:, None]
        del xb, sq, t, acc, rt
    torch.cuda.synchronize()
    off = np.asarray(index.list_offsets, dtype=np.int64)
    lrows = np.asarray(index.list_rows)
    lists = [lrows[off[c]:off[c + 1]] for c in range(kc)]
    ref_corpus = pqv.Corpus.from_device_ptr(nx_t.data_ptr(), n, dim, device=0, keepalive=nx_t)
    ref = pqv.Searcher(normalised_index(pqv, dim, index.centroids, lists), ref_corpus)
    got = _device(torch, s, pqv.PQV_COSINE, q, k, nprobe, flags=True)
    exp = _device(torch, ref, pqv.PQV_L2SQ_REF4, normalise(q), k, nprobe, flags=True)
    _same_topk(got[:4], exp[:4])
    assert (got[4] == exp[4]).all() and (got[2] == k).all()
    _same_topk(s.topk(q[:16], k, nprobe, metric=pqv.PQV_COSINE), ref.topk(normalise(q[:16]), k, nprobe, sqrt_out=False))
    # the torch normalisation of the reference setup is the numpy restatement's
    sample = np.random.default_rng(3).integers(0, n, 256)
    assert (_bits(normalise(x_t[sample].cpu().numpy())) == _bits(nx_t[sample].cpu().numpy())).all()
    s.close(); ref.close(); corpus.close(); ref_corpus.close()
    del x_t, nx_t
    gc.collect()
    torch.cuda.empty_cache()
