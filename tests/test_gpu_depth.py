"""Per-query probe depths on the GPU (pqv_topk_depth / pqv_topk_depth_device; Searcher.topk(probe_depths= | d2_ratio=, max_nprobe=),
topk_device(..., d_nprobe_used=); TopkBuilder.d2_ratio).

The yardstick is never the code under test.  nprobe_used comes from tests/depth_ref.py (numpy over the ORACLE's probe order and its
l2_ref4).  For each distinct expected depth u ONE existing uniform call runs on the whole batch at nprobe = u, and the queries whose
expected depth is u must equal it byte for byte: rows, distance bits, n_found, tie flags, n_candidates.  Host form, device form,
device form with tie flags.  The screened centroid probe by plan_topk's default rule is held to the oracle's topk_batch per
distinct depth instead, and so is every depth mode of tests/mutated_cases.py on mutated indexes, under the forced screen, at far
rows and under every searcher option (test_gpu_mutated_search.py, test_gpu_probe_screen_modes.py, test_gpu_far_rows.py).

Every depth call is preceded by a uniform call at nprobe = P on the same searcher and stream: the scratch slots of the ranks beyond
a query's depth then hold valid-looking entries of the same shape, and a kernel that reads them gives a wrong answer.

Every test asserts its own premise on the REFERENCE's depths before it compares anything; a draw that misses it fails."""
import numpy as np
import pytest

import depth_ref

pytestmark = pytest.mark.gpu

NQ = 16
INF = float("inf")
_SHAPES = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def shape_data(oracle, n, dim, kc, seed, nq=NQ, integer=False):
    """The data recipe of every case (no GPU): rows, queries, the oracle-built index (max_iters 5)."""
    key = (n, dim, kc, seed, nq, integer)
    if key not in _SHAPES:
        rng = np.random.default_rng(seed)
        if integer:
            data = rng.integers(0, 3, (n, dim)).astype(np.float32)
            queries = rng.integers(0, 3, (nq, dim)).astype(np.float32)
        else:
            data = rng.random((n, dim), dtype=np.float32)
            queries = rng.random((nq, dim), dtype=np.float32)
        built = oracle.build_index(data, n_clusters=kc, max_iters=5, workers=1)
        _SHAPES[key] = dict(n=n, dim=dim, data=data, queries=queries, oidx=built, lists=built.lists())
    return _SHAPES[key]


def given_depths(nq, p0, P):
    """0, 1, p0, values in between, P, values above P -- cycled over the batch"""
    vals = [0, 1, p0, (p0 + P) // 2, P, P + 1, 2 ** 32 - 1, p0 + 1, max(P - 1, 1), 1000]
    return np.array([vals[i % len(vals)] for i in range(nq)], np.uint32)


class Dep:
    """shape_data plus the searcher under test (the oracle's centroids and lists)"""

    def __init__(self, pqv, oracle, n, dim, kc, seed, flags=0, **kw):
        d = shape_data(oracle, n, dim, kc, seed, **kw)
        self.__dict__.update(d)
        self.pqv, self.oracle, self.kc = pqv, oracle, len(d["lists"])
        self.corpus = pqv.Corpus.upload(self.data)
        self.s = pqv.Searcher(pqv.Index.from_parts(dim, self.oidx.centroids, self.lists), self.corpus, flags)


def _device(s, q, k, nprobe, flags, metric=0, stream=None, max_nprobe=0, depths=None, ratio=None, used_out=True):
    """topk_device with d2 output -> (rows, dist, n_found, n_candidates, tie flags or None, nprobe_used or None)"""
    import torch
    dev = torch.device("cuda", 0)
    q_t = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(dev)
    nq = len(q)
    r_t = torch.full((nq, k), -1, dtype=torch.int32, device=dev)
    d_t = torch.full((nq, k), float("inf"), dtype=torch.float32, device=dev)
    nf_t = torch.full((nq,), 77, dtype=torch.int32, device=dev)
    nc_t = torch.full((nq,), 77, dtype=torch.int64, device=dev)
    tf_t = torch.full((nq,), 7, dtype=torch.int32, device=dev)
    u_t = torch.full((nq,), 7777, dtype=torch.int32, device=dev)
    kw, keep = {}, None
    if max_nprobe:
        kw.update(max_nprobe=max_nprobe, d_nprobe_used=u_t.data_ptr() if used_out else 0)
        if depths is not None:
            keep = torch.from_numpy(np.asarray(depths, np.uint32).view(np.int32).copy()).to(dev)
            kw["probe_depths"] = keep.data_ptr()
        else:
            kw["d2_ratio"] = ratio
    torch.cuda.synchronize()
    s.topk_device(q_t.data_ptr(), nq, k, nprobe, r_t.data_ptr(), d_t.data_ptr(), nf_t.data_ptr(), nc_t.data_ptr(), sqrt_out=False,
                  metric=metric, d_tie_flags=tf_t.data_ptr() if flags else 0, stream=stream or 0, **kw)
    if stream:
        return r_t, d_t, keep, q_t       # (the caller orders its own work behind the call)
    torch.cuda.synchronize()
    del keep
    return (r_t.cpu().numpy().view(np.uint32), d_t.cpu().numpy(), nf_t.cpu().numpy().astype(np.uint32),
            nc_t.cpu().numpy().astype(np.uint64), tf_t.cpu().numpy() if flags else None,
            u_t.cpu().numpy().astype(np.uint32) if max_nprobe else None)


def _same(got, exp, sel, what):
    for i, name in ((0, "rows"), (1, "dist"), (2, "n_found"), (3, "n_candidates")):
        g, e = np.asarray(got[i])[sel], np.asarray(exp[i])[sel]
        assert g.shape == e.shape and (g.view(np.uint8) == e.view(np.uint8)).all(), f"{what}: {name} differ"


def expected(st, nprobe, max_nprobe, depths=None, ratio=None, metric=0, queries=None):
    q = st.queries if queries is None else queries
    if depths is not None:
        return depth_ref.used_given(depths, nprobe, max_nprobe, st.kc)
    oidx, oq = st.oidx, q
    if metric == 2:
        oidx, oq = depth_ref.cosine_index_and_queries(st.oracle, st.oidx, st.lists, q)
    return depth_ref.used_ratio(st.oracle, oidx, oq, ratio, nprobe, max_nprobe)


def check(st, k, nprobe, max_nprobe, depths=None, ratio=None, metric=0, premise=None, queries=None, what=""):
    """The yardstick of the module's docstring for one depth call; -> (expected nprobe_used, the host form's result)."""
    q = st.queries if queries is None else queries
    exp_used = expected(st, nprobe, max_nprobe, depths, ratio, metric, q)
    what = f"{what} k={k} nprobe={nprobe} max={max_nprobe} ratio={ratio} expected used {exp_used.tolist()}"
    if premise:
        assert premise(exp_used), "premise missed: " + what
    P = min(max_nprobe, st.kc)
    dkw = dict(probe_depths=depths) if depths is not None else dict(d2_ratio=ratio)
    st.s.topk(q, k, P, metric=metric, sqrt_out=False)                                     # poison the lane's scratch
    host = st.s.topk(q, k, nprobe, metric=metric, sqrt_out=False, max_nprobe=max_nprobe, **dkw)
    assert len(host) == 5 and (host[4] == exp_used).all(), f"host nprobe_used {host[4].tolist()}: {what}"
    dev = {}
    for flags in (False, True):
        _device(st.s, q, k, P, flags, metric=metric)                                      # poison
        dev[flags] = _device(st.s, q, k, nprobe, flags, metric=metric, max_nprobe=max_nprobe, depths=depths, ratio=ratio)
        assert (dev[flags][5] == exp_used).all(), f"device nprobe_used {dev[flags][5].tolist()} flags={flags}: {what}"
    for u in sorted(set(exp_used.tolist())):
        sel = exp_used == u
        twin = st.s.topk(q, k, u, metric=metric, sqrt_out=False)
        _same(host, twin, sel, f"host form against the uniform call at nprobe={u}: {what}")
        for flags in (False, True):
            twin_d = _device(st.s, q, k, u, flags, metric=metric)
            _same(dev[flags], twin_d, sel, f"device form flags={flags} against the uniform call at nprobe={u}: {what}")
            if flags:
                assert (dev[True][4][sel] == twin_d[4][sel]).all(), f"tie flags at nprobe={u}: {what}"
    return exp_used, host


def _mixed(u):
    return len(set(u.tolist())) >= 3


def both_kinds(st, k, p0, P, ratio, metric=0, queries=None, what=""):
    """one GIVEN call mixing 0, 1, p0, values between, P and values above it, and one RATIO draw with mixed depths"""
    nq = len(st.queries if queries is None else queries)
    check(st, k, p0, P, depths=given_depths(nq, p0, P), metric=metric, premise=_mixed, queries=queries, what=what + " given")
    check(st, k, p0, P, ratio=ratio, metric=metric, premise=_mixed, queries=queries, what=what + " ratio")


# ---- the shapes and, chosen with the reference on the CPU, the ratios at which each draw has at least three depths ----------------
F16 = dict(n=4096, dim=128, kc=16, seed=139)
I8 = dict(n=4096, dim=256, kc=16, seed=267)
RATIO = {"f16": 1.06, "i8": 1.06, "seq": 1.15, "rows": 1.2, "cos": 1.1, "far": 2.0, "ties": 1.5}


@pytest.fixture(scope="module")
def f16(pqv, oracle):
    return Dep(pqv, oracle, **F16)


@pytest.fixture(scope="module")
def i8(pqv, oracle):
    return Dep(pqv, oracle, **I8)


def test_f16_wide_screen(f16):
    st = f16
    plan = st.s.describe(NQ, 10, 8)
    assert "wide_filter_kernel: f16 screen operands" in plan and "threshold sample 64 rows" in plan, plan
    both_kinds(st, 10, 2, 8, RATIO["f16"], what="f16 screen")


def test_int8_wide_screen(i8):
    st = i8
    plan = st.s.describe(NQ, 10, 8)
    assert "wide_filter_kernel: int8 screen operands" in plan and "threshold sample 64 rows" in plan, plan
    both_kinds(st, 10, 2, 8, RATIO["i8"], what="int8 screen")


@pytest.mark.parametrize("option,route", [("wide_quads", "one quad, 8 waves per block"), ("list_once", "list_filter_kernel")])
def test_int8_256_queries_wide_quads(pqv, oracle, option, route):
    """256 queries: lists gather more pairs than a regular quad takes -- the 160-wide quad instance (wide_quads = 2: whatever the
    previous batch's shape was), or the kernel that reads such a list once (list_once = 1) -- and several quads per list."""
    st = Dep(pqv, oracle, nq=256, **I8)
    st.s.set_option(option, 2 if option == "wide_quads" else 1)
    plan = st.s.describe(256, 10, 8)
    assert "int8 screen operands" in plan and route in plan, plan
    depths = np.array([(8, 7, 8, 6, 8, 9, 3, 8)[i % 8] for i in range(256)], np.uint32)
    u = depth_ref.used_given(depths, 2, 8, st.kc)
    order = np.stack([depth_ref.probe_order(st.oidx, q, 8) for q in st.queries])
    per_list = np.bincount(np.concatenate([order[i, :u[i]] for i in range(256)]), minlength=st.kc)
    assert (per_list > 96).any() and per_list.max() > 160, per_list.tolist()      # premise: wide quads, and a list of several quads
    check(st, 10, 2, 8, depths=depths, premise=_mixed, what=f"256 queries {option}")
    check(st, 10, 2, 8, ratio=RATIO["i8"], premise=_mixed, what=f"256 queries ratio {option}")
    st.s.close()


def test_deferred_evaluation(i8):
    st = i8
    plan = st.s.describe(NQ, 100, 8)
    assert "wide_filter_kernel" in plan and "exact evaluations deferred" in plan, plan       # (k = 100 on 256 dims: f16 operands)
    both_kinds(st, 100, 2, 8, RATIO["i8"], what="deferred")


@pytest.mark.parametrize("option,value,route", [("tile_filter", 0, "tile_rerank_kernel: exact arithmetic"), ("rerank_mode", 2, "tile_"),
                                                ("filter_variant", 1, "tile_rerank_kernel (exact seed window")])
def test_tile_forms(pqv, oracle, option, value, route):
    st = Dep(pqv, oracle, **F16)
    st.s.set_option(option, value)
    if option == "filter_variant":
        st.s.set_option("tile_filter", 2)
    plan = st.s.describe(NQ, 10, 8)
    assert route in plan or (option == "rerank_mode" and "wide_seed_kernel" in plan), plan
    both_kinds(st, 10, 2, 8, RATIO["f16"], what=f"{option}={value}")
    st.s.close()


def test_exact_stream_rerank_mode_1(pqv, oracle):
    st = Dep(pqv, oracle, **F16)
    st.s.set_option("rerank_mode", 1)
    assert "stream_kernel: one candidate stream" in st.s.describe(NQ, 10, 8)
    both_kinds(st, 10, 2, 8, RATIO["f16"], what="rerank_mode=1")
    both_kinds(st, 100, 1, 16, RATIO["f16"], what="rerank_mode=1 k=100")
    st.s.close()


def test_exact_stream_seq_metric(pqv, oracle):
    st = Dep(pqv, oracle, 2048, 32, 4, 43)
    assert "stream_kernel: one candidate stream" in st.s.describe(NQ, 10, 4, pqv.PQV_L2SQ_SEQ)
    both_kinds(st, 10, 1, 4, RATIO["seq"], metric=pqv.PQV_L2SQ_SEQ, what="SEQ")
    st.s.close()


def test_exact_stream_row_order_unaligned(pqv, oracle):
    st = Dep(pqv, oracle, 1500, 30, 12, 41, flags=pqv.PQV_LAYOUT_ROW_ORDER)
    assert "tile_rerank_kernel: exact arithmetic" in st.s.describe(NQ, 10, 12)        # (16 queries share the 12 lists: the exact tile form)
    both_kinds(st, 10, 2, 12, RATIO["rows"], what="row order, 30 dims, tile form")
    st.s.set_option("rerank_mode", 1)
    assert "stream_kernel: one candidate stream" in st.s.describe(NQ, 10, 12)
    both_kinds(st, 10, 2, 12, RATIO["rows"], what="row order, 30 dims")
    st.s.close()


def test_cosine(pqv, oracle):
    st = Dep(pqv, oracle, 2048, 64, 4, 64)
    both_kinds(st, 10, 1, 4, RATIO["cos"], metric=pqv.PQV_COSINE, what="cosine")
    st.s.close()


@pytest.mark.parametrize("shape", ["f16", "i8"])
def test_one_query(f16, i8, shape):
    """nq = 1: the uniform call is the fused probe with its own bucketing; the depth call goes through the general pair sort."""
    st = f16 if shape == "f16" else i8
    assert "wide_filter_kernel" in st.s.describe(1, 10, 8)
    for qi, depth in ((0, 0), (1, 3), (2, 8), (3, 50)):
        q = st.queries[qi:qi + 1]
        check(st, 10, 2, 8, depths=np.array([depth], np.uint32), queries=q, what=f"one query depth {depth}")
    us = [int(expected(st, 1, 8, ratio=RATIO[shape], queries=st.queries[i:i + 1])[0]) for i in range(NQ)]
    assert len(set(us)) >= 3, us
    for u in sorted(set(us))[:3]:
        qi = us.index(u)
        check(st, 10, 1, 8, ratio=RATIO[shape], queries=st.queries[qi:qi + 1], what=f"one query ratio, expected {u}")


def test_one_query_whose_cut_ranks_hold_nearer_seed_rows(pqv, oracle):
    """One query selects its first threshold inside the seed launch, over the bounds of all P ranks: those of the ranks it does not
    walk must read "none" (launch_depth_seed_clear).  The query's nearest list is cut down to its 12 FARTHEST rows -- fewer than
    the seed sample, so the true k-th distance is among the sampled bounds -- and the rows taken out head the second list: after the
    uniform call at nprobe = P the scratch holds bounds of k nearer rows at a rank the depth call cuts."""
    d = shape_data(oracle, **F16)
    k, P, q = 10, 8, d["queries"][:1]
    order = depth_ref.probe_order(d["oidx"], q[0], P)
    c0, c1 = int(order[0]), int(order[1])
    mine = np.asarray(d["lists"][c0], np.int64)
    by_d = mine[np.argsort(((d["data"][mine].astype(np.float64) - q[0]) ** 2).sum(axis=1))]
    far, near = by_d[-12:], by_d[:-12]
    lists = [np.asarray(l, np.uint32) for l in d["lists"]]
    lists[c0] = np.sort(far).astype(np.uint32)
    lists[c1] = np.concatenate([near.astype(np.uint32), lists[c1]])
    d2 = lambda rows: ((d["data"][np.asarray(rows, np.int64)].astype(np.float64) - q[0]) ** 2).sum(axis=1)       # noqa: E731
    assert len(near) >= 64 and np.sort(d2(lists[c1][:64]))[k - 1] < 0.8 * d2(far).min()          # premise: k nearer rows in the cut rank's sample
    st = Dep.__new__(Dep)
    st.pqv, st.oracle, st.kc, st.data, st.lists, st.dim, st.n, st.queries = pqv, oracle, len(lists), d["data"], lists, d["dim"], d["n"], q
    cents = np.asarray(d["oidx"].centroids, np.float32).reshape(-1, d["dim"])
    st.oidx = oracle.index_from_parts(d["dim"], cents, lists)
    st.corpus = pqv.Corpus.upload(d["data"])
    st.s = pqv.Searcher(pqv.Index.from_parts(d["dim"], cents, lists), st.corpus)
    assert "wide_filter_kernel" in st.s.describe(1, k, P)
    _, host = check(st, k, 1, P, depths=np.array([1], np.uint32), premise=lambda u: u[0] == 1, what="one query, short nearest list, given")
    want = st.oidx.topk_batch(d["data"], q, k, 1)
    assert host[2][0] == k == want[2][0] and host[3][0] == 12 and sorted(host[0][0].tolist()) == sorted(want[0][0].tolist())
    check(st, k, 1, P, ratio=1.0, premise=lambda u: u[0] == 1, what="one query, short nearest list, ratio 1")
    st.s.close()


def test_beyond_one_chunk_of_64_ranks(pqv, oracle):
    st = Dep(pqv, oracle, 4096, 32, 200, 77)
    depths = np.array([0, 1, 4, 63, 64, 65, 100, 128, 129, 149, 150, 151, 1000, 2 ** 32 - 1, 70, 5], np.uint32)
    check(st, 20, 4, 150, depths=depths, premise=lambda u: (u < 64).any() and (u > 64).any() and (u > 128).any() and (u == 150).any(), what="200 lists")
    check(st, 20, 4, 150, ratio=RATIO["far"], premise=lambda u: _mixed(u) and (u > 64).any() and (u < 64).any(), what="200 lists ratio")
    check(st, 20, 4, 1000, ratio=INF, premise=lambda u: (u == 200).all(), what="200 lists, every list")
    st.s.close()


# ---- the screened centroid probe by the DEFAULT rule, two probe blocks --------------------------------------------------------------
SCREENED = "probe_screen_kernel + probe_resolve_kernel"
# ratio: the median of d2_40 / d2_0 over the draw's queries, from the reference on the CPU -- 8 queries stay at p0, 92 end below rank
# 64, 18 between 64 and 80, 17 at 80
RULE = dict(n=4096, dim=32, kc=320, nq=128, seed=320, k=10, p0=2, P=80, ratio=1.578)


def rule_data(oracle):
    """320 centroids (two probe blocks of 256; P = 80 = kc / 4, 128 queries: plan_topk's own rule takes the screen), no GPU: uniform
    rows, 320 of them the centroids, the lists by the f64 nearest centroid; three of four queries beside a row, the fourth uniform,
    query 0 IS a centroid."""
    if "rule" not in _SHAPES:
        n, dim, kc, nq = RULE["n"], RULE["dim"], RULE["kc"], RULE["nq"]
        rng = np.random.default_rng(RULE["seed"])
        data = rng.random((n, dim), dtype=np.float32)
        cents = np.ascontiguousarray(data[np.sort(rng.choice(n, kc, replace=False))])
        x, c = data.astype(np.float64), cents.astype(np.float64)
        owner = ((x * x).sum(1)[:, None] - 2.0 * (x @ c.T) + (c * c).sum(1)[None, :]).argmin(axis=1)
        lists = [np.flatnonzero(owner == j).astype(np.uint32) for j in range(kc)]
        queries = rng.random((nq, dim), dtype=np.float32)
        for i in range(nq):
            if i % 4 != 3:
                queries[i] = data[(37 * i) % n] + np.float32(0.05) * (rng.random(dim, dtype=np.float32) - np.float32(0.5))
        queries[0] = cents[kc // 2]
        _SHAPES["rule"] = dict(n=n, dim=dim, data=data, queries=np.ascontiguousarray(queries), cents=cents, lists=lists,
                               oidx=oracle.index_from_parts(dim, cents, lists))
    return _SHAPES["rule"]


def _oracle_answer(d, used, k):
    """the oracle's topk_batch (the heap, sqrt_out) at each distinct depth u for the queries whose depth is u, padded as the library pads"""
    nq = len(used)
    rows, dist = np.full((nq, k), 0xFFFFFFFF, np.uint32), np.full((nq, k), np.inf, np.float32)
    nf, nc = np.zeros(nq, np.uint32), np.zeros(nq, np.uint64)
    for u in sorted(set(used.tolist())):
        for q in np.flatnonzero(used == u):
            r, x, f, c = d["oidx"].topk_batch(d["data"], d["queries"][q:q + 1], k, u)
            rows[q, :f[0]], dist[q, :f[0]], nf[q], nc[q] = r[0, :f[0]], x[0, :f[0]], f[0], c[0]
    return rows, dist, nf, nc


@pytest.mark.parametrize("kind", ["given", "ratio"])
def test_screened_probe_by_the_default_rule(pqv, oracle, monkeypatch, kind):
    """No set_option and no PQV_PROBE_SCREEN: 128 queries, 320 centroids and P = kc / 4 take the screened probe by plan_topk's own
    rule (two probe blocks), and the probe merge behind it hands out the ranks' d2 (MergeArgs::probe_d2).  nprobe_used from
    depth_ref; rows, distance bits, n_found and n_candidates from the oracle's topk_batch per distinct depth; a second searcher
    at probe_screen = 0 agrees byte for byte."""
    monkeypatch.delenv("PQV_PROBE_SCREEN", raising=False)
    d = rule_data(oracle)
    nq, k, p0, P, kc = RULE["nq"], RULE["k"], RULE["p0"], RULE["P"], RULE["kc"]
    q = d["queries"]
    assert P == kc // 4 and kc > 256 and min(len(l) for l in d["lists"]) < k
    if kind == "given":
        vals = [0, 1, 2, 3, 40, 63, 64, 65, 79, 80, 81, 1000, 2 ** 32 - 1, 70, 5, 64]
        depths, ratio = np.array([vals[i % len(vals)] for i in range(nq)], np.uint32), None
        used = depth_ref.used_given(depths, p0, P, kc)
        assert {2, 3, 63, 64, 65, 79, 80} <= set(used.tolist())
    else:
        depths, ratio = None, RULE["ratio"]
        used = depth_ref.used_ratio(oracle, d["oidx"], q, ratio, p0, P)
        at = [int((used == p0).sum()), int((used < 64).sum()), int(((used > 64) & (used < P)).sum()), int((used == P).sum())]
        assert at[0] >= 4 and at[1] >= 32 and at[2] >= 8 and at[3] >= 8 and used[0] == p0, (at, used.tolist())
    want = _oracle_answer(d, used, k)
    assert (want[2] < k).any() and (want[2] == k).any()
    corpus = pqv.Corpus.upload(d["data"])
    dkw = dict(probe_depths=depths) if depths is not None else dict(d2_ratio=ratio)
    got = []
    for option in (None, 0):
        s = pqv.Searcher(pqv.Index.from_parts(d["dim"], d["cents"], d["lists"]), corpus)
        if option is not None:
            s.set_option("probe_screen", option)
        plan = s.describe(nq, k, P)
        assert (SCREENED in plan) == (option is None), plan
        what = f"default rule {kind} probe_screen={option}"
        s.topk(q, k, P, sqrt_out=False)                                                   # poison the lane's scratch
        host = s.topk(q, k, p0, max_nprobe=P, **dkw)
        assert (host[4] == used).all(), f"host nprobe_used {host[4].tolist()}, expected {used.tolist()}: {what}"
        _same(host, want, slice(None), what + ": host form against the oracle")
        _device(s, q, k, P, False)                                                        # poison
        dev = _device(s, q, k, p0, False, max_nprobe=P, depths=depths, ratio=ratio)
        assert (dev[5] == used).all() and (dev[3] == want[3]).all() and (dev[2] == want[2]).all(), what + ": device form"
        got.append((host, dev))
        s.close()
    for a, b in zip(got[0], got[1]):
        for x, y in zip(a, b):
            assert (x is None and y is None) or (np.asarray(x).view(np.uint8) == np.asarray(y).view(np.uint8)).all()
    corpus.close()


# ---- 2 to 7 queries: the per-query stream probe (probe_rows is off below 8 queries), then the general pair sort ------------------------
@pytest.mark.parametrize("nq", [2, 7])
@pytest.mark.parametrize("shape", ["f16", "i8"])
def test_small_batches(f16, i8, shape, nq):
    st = f16 if shape == "f16" else i8
    p0, P = 2, 8
    plan = st.s.describe(nq, 10, P)
    assert "centroid probe: stream_kernel" in plan and "probe_rows_kernel" not in plan and "wide_filter_kernel" in plan, plan
    few = lambda u: len(set(u.tolist())) >= min(nq, 3)                                     # noqa: E731
    depths = np.array([1, 5, 8, 9, 3, 2 ** 32 - 1, 0][:nq], np.uint32)
    check(st, 10, p0, P, depths=depths, premise=few, queries=st.queries[:nq], what=f"{nq} queries given")
    # the ratio draw: the queries ordered so that the first ones have depths of their own
    us = expected(st, p0, P, ratio=RATIO[shape], queries=st.queries).tolist()
    order = [us.index(u) for u in sorted(set(us))]
    order += [i for i in range(NQ) if i not in order]
    check(st, 10, p0, P, ratio=RATIO[shape], premise=few, queries=np.ascontiguousarray(st.queries[order[:nq]]), what=f"{nq} queries ratio")


# ---- clamping to the lists there are ----------------------------------------------------------------------------------------------------
def test_depths_clamp_to_the_lists(pqv, oracle):
    st = Dep(pqv, oracle, 4096, 32, 200, 77)
    every = lambda u: (u == 200).all()                                                     # noqa: E731
    # nprobe above the lists: floor and ceiling are both the 200 lists
    check(st, 20, 300, 1000, depths=given_depths(NQ, 300, 1000), premise=every, what="nprobe > kc, given")
    check(st, 20, 300, 1000, ratio=1.0, premise=every, what="nprobe > kc, ratio")
    # max_nprobe == kc + 1: the ceiling is kc, a given depth of kc + 1 or 2^32 - 1 walks every list
    depths = np.array([(199, 200, 201, 2 ** 32 - 1, 0, 64)[i % 6] for i in range(NQ)], np.uint32)
    check(st, 20, 4, 201, depths=depths, premise=lambda u: set(u.tolist()) == {4, 64, 199, 200}, what="max_nprobe == kc + 1, given")
    check(st, 20, 4, 201, ratio=INF, premise=every, what="max_nprobe == kc + 1, ratio inf")
    st.s.close()


# ---- the rule on special values -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("screen", [None, 0])
def test_ratio_on_nan_and_overflowing_queries(pqv, oracle, screen):
    """an all-NaN query: every comparison is false, so it walks p0 lists; a query of 1e30 components: every d2 is +inf and so is
    t, so it walks all P.  nprobe_used from depth_ref, n_candidates the summed lengths of the lists, rows and distances the
    uniform call's.  probe_screen at its default and at 0."""
    st = Dep(pqv, oracle, **F16)
    if screen is not None:
        st.s.set_option("probe_screen", screen)
    p0, P = 2, 8
    q = st.queries.copy()
    q[5], q[10] = np.nan, np.float32(1e30)
    d2 = depth_ref.probe_d2(oracle, st.oidx, q[10], P)
    assert np.isinf(d2).all() and np.isnan(depth_ref.probe_d2(oracle, st.oidx, q[5], P)).all()
    u, host = check(st, 10, p0, P, ratio=RATIO["f16"], premise=lambda u: u[5] == p0 and u[10] == P and _mixed(np.delete(u, [5, 10])),
                    queries=q, what=f"special values probe_screen={screen}")
    lens = np.array([len(l) for l in st.lists], np.uint64)
    for i in (5, 10):                          # (all distances equal, NaN or +inf: the probe order (d2, id) is by centroid id)
        assert depth_ref.probe_order(st.oidx, q[i], P).tolist() == list(range(P))
    for i in range(NQ):
        assert host[3][i] == lens[depth_ref.probe_order(st.oidx, q[i], int(u[i]))].sum(), i
    st.s.close()


def test_ties(pqv, oracle):
    """integer-valued data, k = 10: the device tie flags are the uniform call's, the host form is its heap replay over the used ranks"""
    st = Dep(pqv, oracle, 3000, 8, 6, 4, integer=True)
    before = st.s.counters()["exact_replays"]
    depths = given_depths(NQ, 2, 6)
    u, _ = check(st, 10, 2, 6, depths=depths, premise=_mixed, what="ties given")
    flagged = np.zeros(NQ, bool)
    for v in sorted(set(u.tolist())):
        flagged |= (u == v) & (_device(st.s, st.queries, 10, v, True)[4] != 0)         # (the UNIFORM call's flags)
    assert (flagged & (u < 6)).any(), (flagged.tolist(), u.tolist())                   # premise: a flagged query below P
    assert st.s.counters()["exact_replays"] > before
    check(st, 10, 1, 6, ratio=RATIO["ties"], premise=lambda u: len(set(u.tolist())) >= 2, what="ties ratio")
    st.s.close()


def _integer_index(pqv, oracle):
    """Index.from_parts over small-integer centroids: every probe distance of an integer query is an exact integer"""
    rng = np.random.default_rng(5)
    cents = np.array([[2, 2, 0, 0], [2, 0, 0, 0], [1, 1, 2, 0], [2, 1, 1, 0], [3, 3, 3, 3], [4, 4, 4, 4], [9, 9, 9, 9], [0, 5, 0, 5]], np.float32)
    data = np.concatenate([c + rng.integers(-1, 2, (300 + 40 * i, 4)) for i, c in enumerate(cents)]).astype(np.float32)
    owner = np.repeat(np.arange(len(cents)), [300 + 40 * i for i in range(len(cents))])
    lists = [np.flatnonzero(owner == c).astype(np.uint32) for c in range(len(cents))]
    st = Dep.__new__(Dep)
    st.pqv, st.oracle, st.kc, st.data, st.lists, st.dim = pqv, oracle, len(cents), data, lists, 4
    st.oidx = oracle.index_from_parts(4, cents, lists)
    st.corpus = pqv.Corpus.upload(data)
    st.s = pqv.Searcher(pqv.Index.from_parts(4, cents, lists), st.corpus)
    return st, cents


def test_ratio_exact_boundary_and_special_values(pqv, oracle):
    st, cents = _integer_index(pqv, oracle)
    q0 = np.zeros(4, np.float32)
    d2 = depth_ref.probe_d2(oracle, st.oidx, q0, 8)
    assert d2[:4].tolist() == [4, 6, 6, 8] and depth_ref.probe_order(st.oidx, q0, 4).tolist() == [1, 2, 3, 0], d2.tolist()
    st.queries = np.stack([q0, cents[0], cents[5] + np.array([0, 0, 0, 1], np.float32), np.array([3, 3, 3, 2], np.float32)] * 4).astype(np.float32)
    # equality decides: both lists tied at 1.5 x the nearest are in, the next one is not
    u, _ = check(st, 10, 1, 8, ratio=1.5, premise=lambda u: u[0] == 3, what="equality at the threshold")
    below = float(np.nextafter(np.float32(1.5), np.float32(0)))
    check(st, 10, 1, 8, ratio=below, premise=lambda u: u[0] == 1, what="one ulp below the threshold")
    check(st, 10, 1, 8, ratio=1.0, premise=lambda u: (u >= 1).all() and u[1] == 1, what="ratio 1")
    check(st, 10, 2, 8, ratio=INF, premise=lambda u: u[0] == 8 and u[1] == 2, what="ratio inf: every list, but a query ON a centroid counts nothing")
    check(st, 10, 1, 8, ratio=1e30, premise=lambda u: u[1] == 1 and u[0] == 8, what="a query equal to a centroid: t == 0")
    check(st, 10, 3, 3, ratio=2.0, premise=lambda u: (u == 3).all(), what="max_nprobe == nprobe")
    st.s.close()


def test_counters_repetition_stream_and_null_used(f16):
    import torch
    st = f16
    k, p0, P = 10, 2, 8
    depths = given_depths(NQ, p0, P)
    u = depth_ref.used_given(depths, p0, P, st.kc)
    assert _mixed(u)
    tot = sum(sum(len(st.lists[c]) for c in depth_ref.probe_order(st.oidx, q, int(p))) for q, p in zip(st.queries, u))
    # the uniform calls' own counting: one call per distinct depth, the queries of that depth
    uni = 0
    for v in sorted(set(u.tolist())):
        uni += int(st.s.topk(st.queries, k, v)[3][u == v].astype(np.int64).sum())
    assert uni == tot
    runs = []
    for call in (lambda: st.s.topk(st.queries, k, p0, sqrt_out=False, max_nprobe=P, probe_depths=depths),
                 lambda: _device(st.s, st.queries, k, p0, False, max_nprobe=P, depths=depths),
                 lambda: _device(st.s, st.queries, k, p0, True, max_nprobe=P, depths=depths)):
        for _ in range(2):
            before = st.s.counters()
            got = call()
            after = st.s.counters()
            assert after["queries"] - before["queries"] == NQ
            assert after["candidate_rows"] - before["candidate_rows"] == tot == int(np.asarray(got[3]).astype(np.int64).sum())
            assert after["embeddings_fetched"] - before["embeddings_fetched"] == tot
            runs.append(got)
    for a, b in zip(runs[0::2], runs[1::2]):
        for x, y in zip(a, b):
            assert (x is None and y is None) or (np.asarray(x).view(np.uint8) == np.asarray(y).view(np.uint8)).all()
    # nprobe_used passed as NULL
    got = _device(st.s, st.queries, k, p0, False, max_nprobe=P, depths=depths, used_out=False)
    assert (got[5] == 7777).all()
    for x, y in zip(got[:4], runs[2][:4]):
        assert (np.asarray(x).view(np.uint8) == np.asarray(y).view(np.uint8)).all()
    raw = st.s.topk(st.queries, k, p0, sqrt_out=False, max_nprobe=P, probe_depths=depths)
    assert (raw[0] == runs[0][0]).all()
    # a caller's stream: poisoned on that stream, and the copy enqueued behind the call on it sees the finished outputs
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        p_r, p_d, _, p_q = _device(st.s, st.queries, k, P, False, stream=stream.cuda_stream)
        r_t, d_t, keep, q_t = _device(st.s, st.queries, k, p0, False, stream=stream.cuda_stream, max_nprobe=P, depths=depths)
        r_c, d_c = r_t.clone(), d_t.clone()
    stream.synchronize()
    assert (r_c.cpu().numpy().view(np.uint32) == runs[2][0]).all() and (_bits(d_c.cpu().numpy()) == _bits(runs[2][1])).all()


def test_refusals_and_builder(f16, pqv, oracle):
    from test_gpu_table import Table
    st = f16
    q = st.queries

    def refused(call, code, text):
        with pytest.raises(pqv.PqvError) as e:
            call()
        assert e.value.code == code and text in str(e.value), (e.value.code, str(e.value))

    uns = "pqv_topk_depth takes k <= 1024 (1023 with tie flags) and at most 1024 probed lists per query"
    refused(lambda: st.s.topk(q, 10, 1, max_nprobe=4, d2_ratio=2.0, metric=pqv.PQV_DOT), -5, "PQV_DOT is not supported by pqv_topk_depth")
    refused(lambda: _device(st.s, q, 10, 1, False, max_nprobe=4, ratio=2.0, metric=pqv.PQV_DOT), -5, "PQV_DOT is not supported by pqv_topk_depth")
    refused(lambda: _device(st.s, q, 1024, 1, True, max_nprobe=4, ratio=2.0), -5, uns)
    refused(lambda: _device(st.s, q, 1025, 1, False, max_nprobe=4, ratio=2.0), -5, uns)
    refused(lambda: st.s.topk(q, 1024, 1, max_nprobe=4, d2_ratio=2.0), -5, uns)          # (the host form always carries tie flags)
    got = _device(st.s, q, 1024, 1, False, max_nprobe=2, depths=np.full(NQ, 2, np.uint32))      # k = 1024 without flags is served
    assert (got[5] == 2).all() and (got[2] <= 1024).all()
    twin = _device(st.s, q, 1024, 2, False)
    _same(got, twin, slice(None), "k = 1024")
    t = Table(pqv, oracle, np.random.default_rng(12), [900, 1400], [4, 6], 32, gap=5)
    tq = np.zeros((2, 32), np.float32)
    refused(lambda: t.s.topk(tq, 10, 1, max_nprobe=2, d2_ratio=2.0), -5, "pqv_topk_depth does not take table searchers")
    refused(lambda: _device(t.s, tq, 10, 1, False, max_nprobe=2, ratio=2.0), -5, "pqv_topk_depth does not take table searchers")
    m = st.s.row_mask(np.ones(st.n, bool))
    refused(lambda: st.s.topk(q, 10, 1, max_nprobe=4, d2_ratio=2.0, mask=m), -5, "do not combine with mask= or keys=")
    m.close()
    refused(lambda: st.s.topk(q, 10, 3, max_nprobe=2, d2_ratio=2.0), -1, "max_nprobe must be >= nprobe")
    refused(lambda: st.s.topk(q, 10, 1, max_nprobe=2, d2_ratio=0.5), -1, "d2_ratio must be >= 1 and not NaN")
    refused(lambda: st.s.topk(q, 0, 1, max_nprobe=2, d2_ratio=2.0), -1, "k must be > 0")
    refused(lambda: st.s.topk(q[:, :100], 10, 1, max_nprobe=2, d2_ratio=2.0), -1, "Query dimension mismatch: expected 128, got 100")
    refused(lambda: st.s.topk(q, 10, 1, max_nprobe=2), -1, "pqv_topk_expand needs a row mask or row keys")      # (existing behaviour)
    # the builder: query 0
    u0 = int(expected(st, 1, 8, ratio=RATIO["f16"], queries=q[:1])[0])
    rows, dist, nf, _ = st.s.topk(q[:1], 10, u0)
    res = pqv.TopkBuilder(st.s, q[0]).k(10).nprobe(1).d2_ratio(RATIO["f16"]).max_nprobe(8).search()
    assert [r.row_idx for r in res] == rows[0, :int(nf[0])].tolist()
    assert (_bits([r.distance for r in res]) == _bits(dist[0, :int(nf[0])])).all()
