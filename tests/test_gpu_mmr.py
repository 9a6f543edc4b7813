"""MMR top-k on the GPU (pqv_mmr_select, pqv_mmr_select_device, pqv_topk_mmr, pqv_topk_mmr_device).

The selection is compared, bit for bit, against the numpy restatement (tests/mmr_ref.py) over the inputs of the key partition tests
(tests/partition_cases.py) and the candidate sets of tests/mmr_cases.py; the fused calls against the calls the contract names as
their twins: pqv_mmr_select_device over the outputs of pqv_topk_device / pqv_topk_masked_device with k = fetch_k.  There are no
tolerances.

The reference forms every pairwise distance in numpy, pick by pick, so the longest selections (n = 1024 with k >= n) run for one
query on the rows of 260 and 768 dimensions and for all five elsewhere."""
import numpy as np
import pytest

import mmr_cases as mc
import mmr_ref as mr
import partition_cases as pc
import partition_ref as pr
import rows_cases as rc
from test_gpu_rows import Setup, long_setup, shape_setup

pytestmark = pytest.mark.gpu

EMPTY = 0xFFFFFFFF
SHAPE_NAMES = ("1500x30", "4096x128", "2048x32-seq")
LONG_NAMES = ("768", "260", "132-cos", "134-dot")


def _same(got, exp, what=""):
    for i, (x, y) in enumerate(zip(got, exp)):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and (x.view(np.uint8) == y.view(np.uint8)).all(), f"{what}: output {i} differs"


def _dev():
    import torch
    return torch.device("cuda", 0)


def _to_dev(a, as_type):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(as_type).copy()).to(_dev())


TAIL = 3


def _outputs(nq, k, with_cand=False):
    """flat outputs with TAIL sentinel slots behind them: rows 7, dist -1, score -2, n_found 7 (n_candidates 7)"""
    import torch
    dev = _dev()
    out = [torch.full((nq * k + TAIL,), 7, dtype=torch.int32, device=dev), torch.full((nq * k + TAIL,), -1.0, dtype=torch.float32, device=dev),
           torch.full((nq * k + TAIL,), -2.0, dtype=torch.float32, device=dev), torch.full((nq + TAIL,), 7, dtype=torch.int32, device=dev)]
    if with_cand:
        out.append(torch.full((nq + TAIL,), 7, dtype=torch.int64, device=dev))
    return out


def _results(out, nq, k):
    """-> (rows u32 [nq, k], dist, score, n_found u32 [, n_candidates u64]); every slot written, nothing behind them"""
    h = [o.cpu().numpy() for o in out]
    assert (h[0][nq * k:] == 7).all() and (h[1][nq * k:] == -1.0).all() and (h[2][nq * k:] == -2.0).all() and (h[3][nq:] == 7).all(), \
        "a call wrote past its outputs"
    rows, dist, score, nf = h[0][:nq * k].view(np.uint32).reshape(nq, k), h[1][:nq * k].reshape(nq, k), h[2][:nq * k].reshape(nq, k), h[3][:nq]
    nf = nf.astype(np.uint32)
    for q in range(nq):      # picks are never sentinels; behind them the padding
        assert nf[q] <= k and (rows[q, nf[q]:] == EMPTY).all() and np.isposinf(dist[q, nf[q]:]).all() and np.isposinf(score[q, nf[q]:]).all()
    res = [rows, dist, score, nf]
    if len(h) > 4:
        assert (h[4][nq:] == 7).all()
        res.append(h[4][:nq].astype(np.uint64))
    return tuple(res)


def select_device(s, cand, rel, k, lam, nf_in=None, metric=0, sqrt_out=False):
    import torch
    cand, rel = np.ascontiguousarray(cand, np.uint32), np.ascontiguousarray(rel, np.float32)
    nq, n = cand.shape
    c_t, r_t = _to_dev(cand, np.int32), _to_dev(rel, np.float32)
    nf_t = _to_dev(np.asarray(nf_in, np.uint32), np.int32) if nf_in is not None else None
    out = _outputs(nq, k)
    torch.cuda.synchronize()
    s.mmr_select_device(c_t.data_ptr(), r_t.data_ptr(), nq, n, k, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(),
                        d_n_found_in=nf_t.data_ptr() if nf_t is not None else 0, lambda_=lam, metric=metric, sqrt_out=sqrt_out)
    torch.cuda.synchronize()
    return _results(out, nq, k)


def fused_device(s, q, k, fetch_k, nprobe, lam, mask=None, metric=0, sqrt_out=False):
    import torch
    q_t = _to_dev(np.asarray(q, np.float32), np.float32)
    out = _outputs(len(q), k, with_cand=True)
    torch.cuda.synchronize()
    s.topk_mmr_device(q_t.data_ptr(), len(q), k, fetch_k, nprobe, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(),
                      out[4].data_ptr(), lambda_=lam, mask=mask, metric=metric, sqrt_out=sqrt_out)
    torch.cuda.synchronize()
    return _results(out, len(q), k)


def stage1_device(s, q, k, nprobe, mask=None, metric=0, sqrt_out=False):
    """topk_device with k = fetch_k -> (rows u32 [nq, k], dist, n_found, n_candidates)"""
    import torch
    nq = len(q)
    q_t = _to_dev(np.asarray(q, np.float32), np.float32)
    dev = _dev()
    out = (torch.full((nq, k), 7, dtype=torch.int32, device=dev), torch.full((nq, k), -1.0, dtype=torch.float32, device=dev),
           torch.full((nq,), 7, dtype=torch.int32, device=dev), torch.full((nq,), 7, dtype=torch.int64, device=dev))
    torch.cuda.synchronize()
    s.topk_device(q_t.data_ptr(), nq, k, nprobe, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), metric=metric,
                  sqrt_out=sqrt_out, mask=mask)
    torch.cuda.synchronize()
    return (out[0].cpu().numpy().view(np.uint32), out[1].cpu().numpy(), out[2].cpu().numpy().astype(np.uint32),
            out[3].cpu().numpy().astype(np.uint64))


def _pairwise(st, sqrt_out):
    return mr.Pairwise(st.kind, st.metric if st.kind == "l2" else pr.REF4, st.data, sqrt_out)


def _sets(st, n, nq, removed=()):
    """name -> [nq] candidate arrays of n ids"""
    near = [mc.nearest(st.d[q], st.kind, st.indexed_rows, n) for q in range(nq)]
    assert all(len(c) == n for c in near)
    return {"stage1": near, "shuffled": [mc.shuffled(c, 40 + q) for q, c in enumerate(near)],
            "dups": [mc.with_duplicates(mc.shuffled(c, 50 + q), 60 + q) for q, c in enumerate(near)],
            "messy": [mc.messy(c, st.n, 70 + q, removed) for q, c in enumerate(near)]}


def _check_select(st, sets, k, lam, sqrt_out, nq, nf_in=None, host=True, what=""):
    """device form == the restatement == host form, for the first nq queries"""
    cand, rel = mc.batch(sets[:nq], st.d, st.kind, sqrt_out)
    exp = mr.select_batch(cand, rel, k, lam, st.indexed, _pairwise(st, sqrt_out), nf_in)
    got = select_device(st.s, cand, rel, k, lam, nf_in, st.metric, sqrt_out)
    _same(got, exp, f"{what} device form vs the restatement")
    if host:
        _same(st.s.mmr_select(cand, rel, k, lambda_=lam, n_found=nf_in, metric=st.metric, sqrt_out=sqrt_out), got, f"{what} host form vs device form")
    return got


def _against_the_restatement(st, removed=()):
    seen_k, seen_lam = set(), set()
    for i, n in enumerate(mc.NS):
        sets = _sets(st, n, st.nq, removed)
        for j, name in enumerate(("stage1", "shuffled", "dups", "messy")):
            kind_k = ("one", "ten", "n", "beyond")[(i + j) % 4]
            k = {"one": 1, "ten": 10, "n": n, "beyond": n + 3}[kind_k]
            lam = mc.LAMBDAS[(i + 3 * j) % 4]
            nq = max(1, min(st.nq, int(1e9 // (min(k, n) * n * st.dim))))      # (the reference's work: picks x candidates x dim)
            sqrt_out = (i % 2 == 0) != (j >= 2)
            what = f"{name} n={n} k={k} lambda={lam} sqrt_out={sqrt_out}"
            rows, dist, score, nf = _check_select(st, sets[name], k, lam, sqrt_out, nq, what=what)
            seen_k.add(kind_k); seen_lam.add(lam)
            for q in range(nq):
                cons = mr.considered(sets[name][q], st.indexed)
                assert nf[q] == min(k, cons.sum()), what
                assert np.isin(rows[q, :nf[q]], np.asarray(sets[name][q])[cons]).all()
            if name == "messy" and n > 3:
                assert (nf < n).all(), "ids that are no rows are never picked"
    assert seen_k >= {"one", "ten", "n", "beyond"} and seen_lam == set(mc.LAMBDAS)


@pytest.fixture(scope="module", params=SHAPE_NAMES)
def shape(request, pqv, oracle):
    return shape_setup(pqv, oracle, request.param)


@pytest.fixture(scope="module", params=LONG_NAMES)
def long_shape(request, pqv, oracle):
    return long_setup(pqv, oracle, request.param)


@pytest.fixture(scope="module")
def s128(pqv, oracle):
    return shape_setup(pqv, oracle, "4096x128")


def test_selection_against_the_restatement(shape):
    """n in {1, 63, 64, 65, 257, 1024}; k 1, 10, n and above the considered count; lambda 0, 0.3, 0.5, 1; REF4 with and without
    sqrt_out and SEQ; candidates in stage-1 order, shuffled, with duplicates, with ids that are no rows; host and device forms"""
    _against_the_restatement(shape)


def test_selection_against_the_restatement_long_rows(long_shape):
    """... rows of several chunks (768: CG 64; 260: stored zero-padded), PQV_COSINE on 132-cos and PQV_DOT on 134-dot"""
    _against_the_restatement(long_shape)


def test_n_found_in_bounds_the_candidates(s128):
    st = s128
    n = 257
    sets = _sets(st, n, st.nq)["shuffled"]
    nf_in = np.array([0, 1, 64, 200, 1000], np.uint32)[:st.nq]            # (beyond n: n)
    for k, lam in ((10, 0.5), (n, 0.3)):
        rows, dist, score, nf = _check_select(st, sets, k, lam, True, st.nq, nf_in=nf_in, what=f"n_found_in k={k}")
        assert (nf == np.minimum(k, np.minimum(nf_in, n))).all()
        for q in range(st.nq):
            assert np.isin(rows[q, :nf[q]], sets[q][:nf_in[q]]).all()


def test_equal_scores_fall_to_the_lower_position(pqv):
    """partition_cases.tie_case(): integer rows, so rel, pd and the scores tie all the time and the position decides"""
    data, queries, _ = pc.tie_case()
    n, dim = data.shape
    lists3 = [np.arange(i, n, 3, dtype=np.uint32) for i in range(3)]
    st = Setup(pqv, data, queries, np.zeros((3, dim), np.float32), lists3, 0, "l2", pr.distances("l2", pr.REF4, data, queries))
    assert any(len(np.unique(row)) < len(row) // 4 for row in st.d), "the case is about equal distances"
    for n_c, k, lam in ((257, 40, 0.5), (257, 257, 0.0), (1024, 30, 0.5), (65, 65, 1.0), (64, 20, 0.3)):
        sets = _sets(st, n_c, st.nq)
        for name in ("stage1", "dups"):
            _check_select(st, sets[name], k, lam, False, st.nq, what=f"ties {name} n={n_c} k={k} lambda={lam}")


@pytest.mark.parametrize("layout", ["ivf", "row", "release"])
@pytest.mark.parametrize("name", ["4096x128", "1500x30"])
def test_layouts(pqv, oracle, layout, name):
    """flags 0, PQV_LAYOUT_ROW_ORDER and PQV_RELEASE_ROW_ORDER read the same rows: the selection, and a cosine selection on the same
    searcher (the cosine layout made by a call that has no queries)"""
    flags = {"ivf": 0, "row": pqv.PQV_LAYOUT_ROW_ORDER, "release": pqv.PQV_RELEASE_ROW_ORDER}[layout]
    st = shape_setup(pqv, oracle, name, flags=flags)
    cos = Setup.__new__(Setup)
    cos.__dict__.update(st.__dict__)
    cos.metric, cos.kind, cos.d = pqv.PQV_COSINE, "cos", pr.distances("cos", pr.REF4, st.data, st.queries)
    for view in (cos, st):
        sets = _sets(view, 257, 3)
        _check_select(view, sets["messy"], 10, 0.3, True, 3, what=f"{layout} {name} {view.kind} messy")
        _check_select(view, sets["stage1"], 65, 0.5, False, 3, what=f"{layout} {name} {view.kind} stage1")


def test_removed_rows_are_not_candidates(pqv, oracle):
    n = pc.SHAPES["1500x30"]["n"]
    removed = np.unique(np.random.default_rng(8).integers(0, n, n // 5))
    st = shape_setup(pqv, oracle, "1500x30", removed=removed)
    for n_c in (65, 1024):
        sets = _sets(st, n_c, st.nq, removed[:9])["messy"]
        sets[0][:min(40, n_c)] = removed[:min(40, n_c)]
        assert np.isin(np.concatenate(sets), removed).any()
        rows, dist, score, nf = _check_select(st, sets, n_c, 0.5, True, 2, what=f"removed n={n_c}")
        assert not np.isin(rows[rows != EMPTY], removed).any() and (nf < n_c).all()
    gone = [removed[:64].astype(np.uint32)] * st.nq
    assert (_check_select(st, gone, 5, 0.5, True, st.nq, what="only removed rows")[3] == 0).all()


def test_appended_and_removed_indexes(pqv, oracle):
    """the states of tests/mutated_cases.py (exact30): rows that joined by an append; rows two removes took out"""
    from test_gpu_mutated_search import Zoo
    zoo = Zoo(pqv, oracle, "exact30", searchers=False)
    c = zoo.case
    corpus = pqv.Corpus.create(c.n1, c.dim)
    try:
        corpus.append(c.X[:c.n0])
        built = pqv.IndexBuilder(corpus).n_clusters(c.kc).max_iters(5).workers(1).build()
        corpus.append(c.X[c.n0:c.n1])
        appended = built.append(corpus)
        for state, index, corp in (("appended", appended, corpus), ("chained", zoo.index["chained"], zoo.corpus)):
            m = c.models[state]
            s = pqv.Searcher(index, corp)
            n = corp.rows
            st = Setup.__new__(Setup)
            indexed, X = np.zeros(n, bool), np.zeros((n, m.dim), np.float32)
            have = min(n, m.n)
            indexed[:have], X[:have] = m.in_lists()[:have], m.X[:have]
            q = c.Q[:3]
            st.__dict__.update(pqv=pqv, s=s, data=X, queries=q, metric=0, kind="l2", d=pr.distances("l2", pr.REF4, X, q), n=n, dim=m.dim, nq=3,
                               indexed=indexed, indexed_rows=np.nonzero(indexed)[0])
            gone = np.nonzero(~indexed)[0][:5]
            n_c = min(257, int(indexed.sum()))
            sets = _sets(st, n_c, 3, gone)
            if state == "appended":
                assert any((np.asarray(x) >= c.n0).any() for x in sets["stage1"]), "appended rows among the candidates"
            _check_select(st, sets["messy"], 20, 0.5, True, 3, what=f"{state} messy")
            _check_select(st, sets["stage1"], n_c, 0.3, True, 3, what=f"{state} stage1")
            # ... and the fused call on that state against its twin
            stage = stage1_device(s, q, 64, 2, sqrt_out=True)
            _same(fused_device(s, q, 10, 64, 2, 0.5, sqrt_out=True)[:4], select_device(s, stage[0], stage[1], 10, 0.5, stage[2], 0, True),
                  f"{state} fused vs its twin")
            s.close()
        appended.close()
        built.close()
    finally:
        corpus.close()
        zoo.close()


@pytest.mark.parametrize("nq", [1, 5, 130])
def test_batches_of_1_5_and_130_queries(s128, nq):
    """the selection device form against the restatement for every query of the batch, the host form against the device form"""
    st = s128
    near = [mc.nearest(st.d[q % st.nq], "l2", st.indexed_rows, 65) for q in range(nq)]
    cand = np.stack([mc.shuffled(c, 90 + q) for q, c in enumerate(near)])
    rel = np.stack([mc.rel_of(c, st.d[q % st.nq], "l2", True) for q, c in enumerate(cand)])
    nf_in = (np.arange(nq) * 7 % 66).astype(np.uint32)
    exp = mr.select_batch(cand, rel, 10, 0.5, st.indexed, _pairwise(st, True), nf_in)
    got = select_device(st.s, cand, rel, 10, 0.5, nf_in, 0, True)
    _same(got, exp, f"nq={nq}")
    _same(st.s.mmr_select(cand, rel, 10, lambda_=0.5, n_found=nf_in), got, f"nq={nq} host form")
    q = np.tile(st.queries, (nq // st.nq + 1, 1))[:nq]
    f = fused_device(st.s, q, 10, 100, 3, 0.5, sqrt_out=True)
    _same(st.s.topk_mmr(q, 10, 100, 3, lambda_=0.5), f, f"nq={nq} fused host form vs device form")


def test_host_selection_across_a_sub_batch(s128):
    """The host form cuts its queries where 8 n + 12 k + 8 bytes per query reach 64 MiB: with n = 64 and k = 3000 that is 1837
    queries, so 1840 cross it once.  The device form is the twin; the restatement checks the queries around the cut."""
    st = s128
    n, k, nq = 64, 3000, 1840
    cut = (1 << 26) // (8 * n + 12 * k + 8)
    assert 1 < cut < nq
    base = [mc.nearest(st.d[q], "l2", st.indexed_rows, n) for q in range(st.nq)]
    cand = np.stack([mc.shuffled(base[q % st.nq], 1000 + q) for q in range(nq)])
    rel = np.stack([mc.rel_of(c, st.d[q % st.nq], "l2", True) for q, c in enumerate(cand)])
    nf_in = (np.arange(nq) % (n + 1)).astype(np.uint32)
    got = select_device(st.s, cand, rel, k, 0.5, nf_in, 0, True)
    _same(st.s.mmr_select(cand, rel, k, lambda_=0.5, n_found=nf_in), got, "host form across its sub-batch vs device form")
    assert (got[3] == nf_in).all()
    pick = [0, cut - 1, cut, cut + 1, nq - 1]
    exp = mr.select_batch(cand[pick], rel[pick], k, 0.5, st.indexed, _pairwise(st, True), nf_in[pick])
    _same([g[pick] for g in got], exp, "the queries around the cut vs the restatement")


FUSED = (("4096x128", 3), ("132-cos", 2), ("134-dot", 2), ("2048x32-seq", 2))


@pytest.fixture(scope="module", params=FUSED, ids=[f[0] for f in FUSED])
def fused_case(request, pqv, oracle):
    name, nprobe = request.param
    return (long_setup if name in pc.LONG_SHAPES else shape_setup)(pqv, oracle, name), nprobe


def test_fused_call_equals_selection_over_stage_one(fused_case):
    """pqv_topk_mmr_device == pqv_mmr_select_device over pqv_topk_device(k = fetch_k), with and without a mask; the host form equals
    the device form; lambda = 1 gives stage 1's first k columns; the whole chain equals the restatement over stage 1's outputs"""
    st, nprobe = fused_case
    allow = np.random.default_rng(3).random(st.n) < 0.5
    mask = st.s.row_mask(allow)
    try:
        for m in (None, mask):
            for fetch_k, k, lam, sqrt_out in ((100, 10, 0.5, True), (1024, 10, 0.3, False), (65, 65, 0.0, True), (64, 1, 0.5, False)):
                what = f"{st.kind} fetch_k={fetch_k} k={k} lambda={lam} mask={m is not None}"
                stage = stage1_device(st.s, st.queries, fetch_k, nprobe, m, st.metric, sqrt_out)
                twin = select_device(st.s, stage[0], stage[1], k, lam, stage[2], st.metric, sqrt_out)
                f = fused_device(st.s, st.queries, k, fetch_k, nprobe, lam, m, st.metric, sqrt_out)
                _same(f[:4], twin, f"{what}: fused vs selection over stage 1")
                assert (f[4] == stage[3]).all(), "n_candidates is stage 1's"
                h = st.s.topk_mmr(st.queries, k, fetch_k, nprobe, lambda_=lam, mask=m, metric=st.metric, sqrt_out=sqrt_out)
                _same(h, f, f"{what}: host form vs device form")
                exp = mr.select_batch(stage[0], stage[1], k, lam, st.indexed, _pairwise(st, sqrt_out), stage[2])
                _same(twin, exp, f"{what}: selection over stage 1 vs the restatement")
                if m is not None:
                    assert allow[f[0][f[0] != EMPTY]].all()
            one = fused_device(st.s, st.queries, 10, 100, nprobe, 1.0, m, st.metric, True)
            stage = stage1_device(st.s, st.queries, 100, nprobe, m, st.metric, True)
            _same([one[0], one[1], one[3]], [stage[0][:, :10], stage[1][:, :10], np.minimum(stage[2], 10)], "lambda = 1 vs stage 1's first k")
    finally:
        mask.close()


def test_searcher_options_leave_the_fused_result(s128):
    st = s128
    base = fused_device(st.s, st.queries, 10, 100, 3, 0.5, sqrt_out=True)
    try:
        for mode in (1, 2):
            st.s.set_option("rerank_mode", mode)
            _same(fused_device(st.s, st.queries, 10, 100, 3, 0.5, sqrt_out=True), base, f"rerank_mode {mode}")
            _same(st.s.topk_mmr(st.queries, 10, 100, 3, lambda_=0.5), base, f"rerank_mode {mode} host form")
    finally:
        st.s.set_option("rerank_mode", 0)


def test_selection_composes_with_other_search_modes(s128, pqv):
    """mmr_select over the outputs of topk_rows and topk_partition, n_found included"""
    st = s128
    lists = rc.messy_lists(st.n, (65, 255, 30, 257, 1000), 23)
    values = pc.columns(st.n, 5000 + st.dim + 17)["t3"][0]
    col = pqv.Column.upload(values)
    part = st.s.key_partition(col)
    try:
        outs = (("topk_rows", st.s.topk_rows(st.queries, 64, lists, sqrt_out=True)[:3]),
                ("topk_partition", st.s.topk_partition(st.queries, 100, part, query_keys=[-5, 0, 7, 3, 7][:st.nq], sqrt_out=True)[:3]))
        for label, (rows, dist, nf) in outs:
            assert (nf < rows.shape[1]).any(), "a query with fewer results than slots"
            exp = mr.select_batch(rows, dist, 10, 0.5, st.indexed, _pairwise(st, True), nf)
            _same(st.s.mmr_select(rows, dist, 10, lambda_=0.5, n_found=nf), exp, f"mmr_select over {label}")
            _same(select_device(st.s, rows, dist, 10, 0.5, nf, 0, True), exp, f"mmr_select_device over {label}")
    finally:
        part.close()
        col.close()


def test_counters_and_builder(s128, pqv):
    st = s128
    cand, rel = mc.batch(_sets(st, 64, st.nq)["stage1"], st.d, "l2", True)
    select_device(st.s, cand, rel, 10, 0.5, None, 0, True)      # (a searcher's first call builds its row map: one more launch)
    before = st.s.counters()
    select_device(st.s, cand, rel, 10, 0.5, None, 0, True)
    after = st.s.counters()
    assert after["queries"] - before["queries"] == st.nq and after["kernel_launches"] - before["kernel_launches"] == 1
    assert all(after[c] == before[c] for c in ("candidate_rows", "embeddings_fetched", "exact_replays"))
    # the fused call counts as its stage 1 does, plus the selection's launch
    b0 = st.s.counters()
    stage1_device(st.s, st.queries, 100, 3, sqrt_out=True)
    b1 = st.s.counters()
    fused_device(st.s, st.queries, 10, 100, 3, 0.5, sqrt_out=True)
    b2 = st.s.counters()
    for c in ("queries", "candidate_rows", "embeddings_fetched", "exact_replays"):
        assert b2[c] - b1[c] == b1[c] - b0[c], c
    assert b2["kernel_launches"] - b1["kernel_launches"] == b1["kernel_launches"] - b0["kernel_launches"] + 1
    # the builder: one query, pick order, where() through the mask
    exp = st.s.topk_mmr(st.queries[:1], 5, 50, 3, lambda_=0.3)
    res = pqv.TopkBuilder(st.s, st.queries[0]).k(5).nprobe(3).mmr(50, lambda_=0.3).search()
    assert [r.row_idx for r in res] == exp[0][0].tolist() and [r.distance for r in res] == exp[1][0].tolist()
    allow = np.random.default_rng(5).random(st.n) < 0.3
    res = pqv.TopkBuilder(st.s, st.queries[0]).k(5).nprobe(3).where(allow).mmr(50).search()
    m = st.s.row_mask(allow)
    try:
        assert [r.row_idx for r in res] == st.s.topk_mmr(st.queries[:1], 5, 50, 3, mask=m)[0][0].tolist() and allow[[r.row_idx for r in res]].all()
    finally:
        m.close()
