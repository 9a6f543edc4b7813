"""Expanding filtered top-k on the GPU (pqv_topk_expand / pqv_topk_expand_device; Searcher.topk(max_nprobe=) /
topk_device(max_nprobe=, d_nprobe_used=); TopkBuilder.max_nprobe).

The yardstick is never the code under test.  nprobe_used comes from tests/expand_ref.py (numpy over the ORACLE's probe order).
For each distinct expected value u ONE existing twin call (mask= / keys= without max_nprobe) runs on the whole batch with nprobe = u,
and the queries whose expected depth is u must equal it bit for bit: rows, distance bits, n_found, tie flags; n_candidates is
the unmasked call's at nprobe = u.  Host form, device form, device form with tie flags.

Every test asserts its own premise on the REFERENCE's depths before it compares anything; a draw that misses it fails."""
import collections

import numpy as np
import pytest

import expand_ref
import key_filter_ref as kf

pytestmark = pytest.mark.gpu

NQ = 16
SELS = ("1/64", "1/8", "1/2")
Flt = collections.namedtuple("Flt", "kind a b")      # a per-query filter's arrays as Python ints (tests/key_filter_ref.py)

_SHAPES = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def shape_data(oracle, n, dim, kc, seed, integer=False, sels=SELS):
    """The data recipe of every case (no GPU): rows, 16 queries, the oracle-built index (max_iters 5), then the masks drawn from the
    same generator in the order of `sels` (1/64, 1/8, 1/2)."""
    key = (n, dim, kc, seed, integer, tuple(sels))
    if key not in _SHAPES:
        rng = np.random.default_rng(seed)
        if integer:
            data = rng.integers(0, 3, (n, dim)).astype(np.float32)
            queries = rng.integers(0, 3, (NQ, dim)).astype(np.float32)
        else:
            data = rng.random((n, dim), dtype=np.float32)
            queries = rng.random((NQ, dim), dtype=np.float32)
        built = oracle.build_index(data, n_clusters=kc, max_iters=5, workers=1)
        masks = {}
        for sel in sels:
            num, den = sel.split("/")
            masks[sel] = rng.random(n) < int(num) / int(den)
        _SHAPES[key] = dict(n=n, dim=dim, data=data, queries=queries, built=built, lists=built.lists(), masks=masks, rng=rng)
    return _SHAPES[key]


class Exp:
    """shape_data plus the searcher under test (the oracle's centroids and lists)"""

    def __init__(self, pqv, oracle, n, dim, kc, seed, flags=0, **kw):
        d = shape_data(oracle, n, dim, kc, seed, **kw)
        self.__dict__.update(d)
        self.pqv, self.oracle, self.oidx, self.kc = pqv, oracle, d["built"], len(d["lists"])
        self.corpus = pqv.Corpus.upload(self.data)
        self.s = pqv.Searcher(pqv.Index.from_parts(dim, self.oidx.centroids, self.lists), self.corpus, flags)
        self.order_q = self.queries      # what the reference's probe order is taken for (cosine: the normalised queries)


def _dev_kw(kw):
    """a host call's filter keywords -> topk_device's (device pointers) and the tensors that back them"""
    import torch
    dev = torch.device("cuda", 0)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=dt)).to(dev)
    out, keep = {}, []
    for name, v in kw.items():
        if name == "query_keys":
            t = up(v, np.int64); keep.append(t); out[name] = t.data_ptr()
        elif name == "query_key_ranges":
            lo, hi = up(v[0], np.int64), up(v[1], np.int64); keep += [lo, hi]; out[name] = (lo.data_ptr(), hi.data_ptr())
        elif name == "query_key_sets":
            lims, vals = kf.sets_to_csr(v)
            tl = up(np.asarray(lims, np.uint64).view(np.int64), np.int64)
            tv = up(np.concatenate([np.asarray(vals, np.int64), np.zeros(1, np.int64)]), np.int64)
            keep += [tl, tv]; out[name] = (tl.data_ptr(), tv.data_ptr())
        else:
            out[name] = v
    return out, keep


def _device(s, q, k, nprobe, flags, kw, max_nprobe=0, metric=0, stream=None):
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
    dkw, keep = _dev_kw(kw)
    if max_nprobe:
        dkw.update(max_nprobe=max_nprobe, d_nprobe_used=u_t.data_ptr())
    torch.cuda.synchronize()
    s.topk_device(q_t.data_ptr(), nq, k, nprobe, r_t.data_ptr(), d_t.data_ptr(), nf_t.data_ptr(), nc_t.data_ptr(), sqrt_out=False,
                  metric=metric, d_tie_flags=tf_t.data_ptr() if flags else 0, stream=stream or 0, **dkw)
    if stream:
        return r_t, d_t, keep       # (the caller orders its own work behind the call)
    torch.cuda.synchronize()
    del keep
    return (r_t.cpu().numpy().view(np.uint32), d_t.cpu().numpy(), nf_t.cpu().numpy().astype(np.uint32),
            nc_t.cpu().numpy().astype(np.uint64), tf_t.cpu().numpy() if flags else None,
            u_t.cpu().numpy().astype(np.uint32) if max_nprobe else None)


def _same_rows(got, exp, sel, what):
    for i, name in enumerate(("rows", "dist", "n_found")):
        g, e = np.asarray(got[i])[sel], np.asarray(exp[i])[sel]
        assert g.shape == e.shape and (g.view(np.uint8) == e.view(np.uint8)).all(), f"{what}: {name} differ"


def check(st, M, kw, k, nprobe, max_nprobe, metric=0, premise=None, oidx=None, what=""):
    """The yardstick of the module's docstring for one expanding call; -> (expected nprobe_used, the host form's result)."""
    q = st.queries
    exp_used = expand_ref.used_for_batch(oidx or st.oidx, st.lists, M, st.order_q, k, nprobe, max_nprobe)
    what = f"{what} k={k} nprobe={nprobe} max={max_nprobe} expected used {exp_used.tolist()}"
    if premise:
        assert premise(exp_used), "premise missed: " + what
    host = st.s.topk(q, k, nprobe, metric=metric, sqrt_out=False, max_nprobe=max_nprobe, **kw)
    assert len(host) == 5 and (host[4] == exp_used).all(), f"host nprobe_used {host[4].tolist()}: {what}"
    dev = {flags: _device(st.s, q, k, nprobe, flags, kw, max_nprobe=max_nprobe, metric=metric) for flags in (False, True)}
    for flags in (False, True):
        assert (dev[flags][5] == exp_used).all(), f"device nprobe_used {dev[flags][5].tolist()} flags={flags}: {what}"
    for u in sorted(set(exp_used.tolist())):
        sel = exp_used == u
        nc_plain = st.s.topk(q, 1, u, metric=metric)[3]
        twin = st.s.topk(q, k, u, metric=metric, sqrt_out=False, **kw)
        _same_rows(host, twin, sel, f"host form against its twin at nprobe={u}: {what}")
        assert (host[3][sel] == nc_plain[sel]).all(), f"host n_candidates at nprobe={u}: {what}"
        for flags in (False, True):
            twin_d = _device(st.s, q, k, u, flags, kw, metric=metric)
            _same_rows(dev[flags], twin_d, sel, f"device form flags={flags} against its twin at nprobe={u}: {what}")
            assert (dev[flags][3][sel] == nc_plain[sel]).all(), f"device n_candidates at nprobe={u}: {what}"
            if flags:
                assert (dev[True][4][sel] == twin_d[4][sel]).all(), f"tie flags at nprobe={u}: {what}"
    return exp_used, host


@pytest.fixture(scope="module")
def shape1(pqv, oracle):
    """4096 x 128, 16 lists, seed 139: CG = 32, lists of 2 .. 1010 rows whose beginnings are not 64-aligned"""
    st = Exp(pqv, oracle, 4096, 128, 16, 139)
    st.rowmasks = {sel: st.s.row_mask(st.masks[sel]) for sel in SELS}
    return st


def _mixed(u, p0=1):
    return len(set(u.tolist())) >= 3 and (u == p0).any()


@pytest.mark.parametrize("sel,k", [("1/64", 10), ("1/8", 100)])
def test_mixed_depths_in_one_batch(shape1, sel, k):
    """Case 1: at least three different depths in one batch, one of them p0."""
    st = shape1
    check(st, st.masks[sel], dict(mask=st.rowmasks[sel]), k, 1, 16, premise=_mixed, what=f"sel {sel}")


def test_almost_nothing_expands_and_the_clamps(shape1):
    """Case 1, rest: sel 1/2 at k in {1, 10, 100}; max_nprobe == nprobe is the twin call; max_nprobe = 1000 is clamped to 16."""
    st = shape1
    for k in (1, 10, 100):
        check(st, st.masks["1/2"], dict(mask=st.rowmasks["1/2"]), k, 1, 16, what="sel 1/2")
    for sel, k, nprobe in (("1/64", 10, 1), ("1/64", 10, 3), ("1/8", 100, 16)):
        check(st, st.masks[sel], dict(mask=st.rowmasks[sel]), k, nprobe, nprobe, premise=lambda u, p=nprobe: (u == p).all(),
              what=f"max == nprobe, sel {sel}")
    a, ha = check(st, st.masks["1/64"], dict(mask=st.rowmasks["1/64"]), 10, 1, 1000, premise=_mixed, what="max 1000")
    b, hb = check(st, st.masks["1/64"], dict(mask=st.rowmasks["1/64"]), 300, 1, 1000, premise=lambda u: (u == 16).all(), what="max 1000, short")
    assert (hb[2] < 300).all() and (hb[2] == st.masks["1/64"][np.concatenate(st.lists).astype(np.int64)].sum()).all()


@pytest.mark.parametrize("layout", ["ivf_ordered", "row_order"])
def test_unaligned_rows_and_short_queries(pqv, oracle, layout):
    """Case 2: 1500 x 30 (dim % 4 != 0), 12 lists, seed 41, both layouts; a batch with short (n_found < k, used == P) and
    satisfied queries; a batch in which every query is short."""
    st = Exp(pqv, oracle, 1500, 30, 12, 41, flags=pqv.PQV_LAYOUT_ROW_ORDER if layout == "row_order" else pqv.PQV_LAYOUT_IVF_ORDERED)
    m64, m8 = st.s.row_mask(st.masks["1/64"]), st.s.row_mask(st.masks["1/8"])
    check(st, st.masks["1/64"], dict(mask=m64), 10, 1, 12, premise=lambda u: len(set(u.tolist())) >= 3, what="sel 1/64")
    cnt = np.array([expand_ref.prefix_counts(st.oidx, st.lists, st.masks["1/8"], q, 6)[-1] for q in st.queries])
    assert (cnt < 100).any() and (cnt >= 100).any(), cnt.tolist()          # premise: short and satisfied queries in one batch
    u, host = check(st, st.masks["1/8"], dict(mask=m8), 100, 2, 6, premise=lambda u: (u == 6).any() and (u < 6).any(), what="sel 1/8")
    short = cnt < 100
    assert (u[short] == 6).all() and (host[2][short] == cnt[short]).all() and (host[2][~short] == 100).all()
    u, host = check(st, st.masks["1/64"], dict(mask=m64), 100, 1, 12, premise=lambda u: (u == 12).all(), what="all short")
    assert (host[2] < 100).all()
    m64.close(); m8.close(); st.s.close()


def test_seq_metric(pqv, oracle):
    """Case 3a: PQV_L2SQ_SEQ on 2048 x 32, 4 lists (the CG = 16 SEQ instantiation)."""
    st = Exp(pqv, oracle, 2048, 32, 4, 43)
    for sel, k in (("1/64", 10), ("1/8", 100)):
        m = st.s.row_mask(st.masks[sel])
        check(st, st.masks[sel], dict(mask=m), k, 1, 4, metric=pqv.PQV_L2SQ_SEQ, premise=lambda u: len(set(u.tolist())) >= 2, what=f"SEQ sel {sel}")
        m.close()
    st.s.close()


def test_wide_rows_and_k_300(pqv, oracle):
    """Case 3b: 2048 x 256, 8 lists, seed 267 (CG = 64): k = 100 at sel 1/8, and k = 300 (S = 16) at sel 1/2."""
    st = Exp(pqv, oracle, 2048, 256, 8, 267)
    m = st.s.row_mask(st.masks["1/8"])
    check(st, st.masks["1/8"], dict(mask=m), 100, 1, 8, premise=lambda u: len(set(u.tolist())) >= 3, what="k 100")
    m.close()
    m = st.s.row_mask(st.masks["1/2"])
    _, host = check(st, st.masks["1/2"], dict(mask=m), 300, 1, 8, premise=lambda u: len(set(u.tolist())) >= 2 and (u < 8).all(), what="k 300")
    assert (host[2] == 300).all()
    m.close(); st.s.close()


def test_cosine(pqv, oracle):
    """Case 3c: PQV_COSINE -- the depth rule over the cosine layout's probe order (normalised centroids, normalised queries)."""
    from cosine_ref import normalise
    st = Exp(pqv, oracle, 2048, 64, 4, 64)
    n_oidx = oracle.index_from_parts(64, normalise(np.asarray(st.oidx.centroids, np.float32).reshape(-1, 64)), st.lists)
    st.order_q = normalise(st.queries)
    m = st.s.row_mask(st.masks["1/64"])
    check(st, st.masks["1/64"], dict(mask=m), 10, 1, 4, metric=pqv.PQV_COSINE, oidx=n_oidx, premise=lambda u: len(set(u.tolist())) >= 2, what="cosine")
    m.close(); st.s.close()


@pytest.mark.parametrize("k", [1, 10, 65])
def test_exact_boundary(shape1, k):
    """Case 4: query 0 finds exactly k - 1 allowed rows in its first list (its position 0 and its last position among them: the
    funnel-shifted first word and the clipped last window), none in its second, one in its third: used == 3.  One more row of
    the first list: used == 1."""
    st = shape1
    order = expand_ref.probe_order(st.oidx, st.queries[0], 3)
    first, second, third = (np.asarray(st.lists[c]).astype(np.int64) for c in order)
    assert len(first) >= k + 1 and len(third) >= 1 and int(st.oidx.list_off[order[0]]) % 64 != 0, (len(first), order.tolist())
    allowed = st.masks["1/8"].copy()
    allowed[first] = False; allowed[second] = False; allowed[third] = False
    if k - 1 >= 2:
        inner = first[1:-1][:: max(1, (len(first) - 2) // (k - 3))][:k - 3] if k > 3 else first[:0]
        allowed[first[0]] = allowed[first[-1]] = True
        allowed[inner] = True
    assert int(allowed[first].sum()) == k - 1
    allowed[third[len(third) // 2]] = True
    m = st.s.row_mask(allowed)
    u, host = check(st, allowed, dict(mask=m), k, 1, 16, premise=lambda u: u[0] == 3, what="k - 1 rows in the first list")
    assert host[2][0] == k
    m.close()
    spare = first[~allowed[first]]
    allowed[spare[len(spare) // 2]] = True
    m = st.s.row_mask(allowed)
    check(st, allowed, dict(mask=m), k, 1, 16, premise=lambda u: u[0] == 1, what="k rows in the first list")
    m.close()


def test_beyond_one_chunk_of_64_ranks(pqv, oracle):
    """Case 5: 4096 x 32, 200 lists, seed 77, a 1/128 mask (35 allowed rows): depths on both sides of rank 64, beyond rank 128, and nprobe 4, max 150."""
    st = Exp(pqv, oracle, 4096, 32, 200, 77, sels=("1/128",))
    M = st.masks["1/128"]
    m = st.s.row_mask(M)
    check(st, M, dict(mask=m), 20, 1, 200, premise=lambda u: (u < 64).any() and (u > 64).any(), what="k 20")
    check(st, M, dict(mask=m), K_BEYOND_128, 1, 200, premise=lambda u: (u > 128).any() and (u < 200).any(), what="beyond 128")
    check(st, M, dict(mask=m), 20, 4, 150, premise=lambda u: (u > 64).any(), what="nprobe 4 max 150")
    m.close(); st.s.close()


K_BEYOND_128 = 30        # (chosen with the reference on the CPU: this draw has depths beyond rank 128 at k = 30)


def _tenant_filters(kind, absent=99):
    """16 per-query filters over tenants [0, 32): different keys per query; query 3 asks for a key no row has; IN: query 5's
    slice is empty."""
    if kind == kf.EQ:
        a = [(5 * i + 1) % 32 for i in range(NQ)]
        a[3] = absent
        return Flt(kf.EQ, a, None)
    if kind == kf.RANGE:
        lo = [(3 * i) % 30 for i in range(NQ)]
        hi = [l + (i % 3) for i, l in enumerate(lo)]
        lo[3] = hi[3] = absent
        return Flt(kf.RANGE, lo, hi)
    sets = [sorted({(7 * i) % 32, (7 * i + 11) % 32, (3 * i + 2) % 32})[: 1 + i % 3] for i in range(NQ)]
    sets[3] = [absent, absent + 1]
    sets[5] = []
    lims, vals = kf.sets_to_csr(sets)
    return Flt(kf.IN, [int(x) for x in lims], [int(x) for x in vals])


def _host_kw(flt):
    if flt.kind == kf.EQ:
        return {"query_keys": np.array(flt.a, np.int64)}
    if flt.kind == kf.RANGE:
        return {"query_key_ranges": (np.array(flt.a, np.int64), np.array(flt.b, np.int64))}
    return {"query_key_sets": [flt.b[flt.a[i]:flt.a[i + 1]] for i in range(len(flt.a) - 1)]}


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
@pytest.mark.parametrize("kind", [kf.EQ, kf.RANGE, kf.IN])
def test_per_query_filters(shape1, dtype, kind):
    """Case 6: a tenant column (1/10 NULL) under PQV_KEY_EQ / RANGE / IN, with and without a shared mask."""
    st = shape1
    rng = np.random.default_rng(600 + kind)
    values = rng.integers(0, 32, st.n).astype(dtype)
    valid = (rng.random(st.n) >= 1 / 10).astype(np.uint8)
    column = st.pqv.Column.upload(values, valid, device=0)
    keys = st.s.row_keys(column)
    column.close()
    flt = _tenant_filters(kind)
    for shared, rowmask in ((None, None), (st.masks["1/2"], st.rowmasks["1/2"])):
        M = np.stack([kf.allowed_for(values, valid, flt.kind, flt.a, flt.b, i, shared) for i in range(NQ)])
        kw = dict(keys=keys, **_host_kw(flt))
        if rowmask is not None:
            kw["mask"] = rowmask
        u, host = check(st, M, kw, 10, 1, 16, premise=lambda u: len(set(u.tolist())) >= 3, what=f"kind {kind} shared {shared is not None}")
        empty = [3, 5] if kind == kf.IN else [3]
        assert (u[empty] == 16).all() and (host[2][empty] == 0).all() and (host[0][empty] == 0xFFFFFFFF).all()
    keys.close()


def test_ties(pqv, oracle):
    """Case 7: integer-valued data, k = 10: the device tie flags are the twin's, the host form is the host twin's heap replay; at
    least one flagged query went beyond p0."""
    st = Exp(pqv, oracle, 3000, 8, 6, 4, integer=True)
    M = st.masks["1/64"]
    m = st.s.row_mask(M)
    before = st.s.counters()["exact_replays"]
    u, _ = check(st, M, dict(mask=m), 10, 1, 6, premise=lambda u: (u > 1).any(), what="ties")
    flagged = np.zeros(NQ, bool)
    for v in sorted(set(u.tolist())):
        flagged |= (u == v) & (_device(st.s, st.queries, 10, v, True, dict(mask=m))[4] != 0)         # (the TWIN's flags)
    assert (flagged & (u > 1)).any(), (flagged.tolist(), u.tolist())
    assert st.s.counters()["exact_replays"] > before
    m.close(); st.s.close()


def test_counters_repetition_and_stream_order(shape1):
    """Case 8: counters advance as for the nq twin calls; a second submission is bit-equal; work that follows a device call on
    the caller's stream reads finished outputs."""
    import torch
    st = shape1
    M, m = st.masks["1/64"], st.rowmasks["1/64"]
    k, nprobe, mx = 10, 1, 16
    u = expand_ref.used_for_batch(st.oidx, st.lists, M, st.queries, k, nprobe, mx)
    assert _mixed(u)
    tot = sum(expand_ref.n_candidates(st.oidx, st.lists, q, int(p)) for q, p in zip(st.queries, u))
    cons = sum(int(expand_ref.prefix_counts(st.oidx, st.lists, M, q, int(p))[-1]) for q, p in zip(st.queries, u))
    runs = []
    for call in (lambda: st.s.topk(st.queries, k, nprobe, sqrt_out=False, mask=m, max_nprobe=mx),
                 lambda: _device(st.s, st.queries, k, nprobe, False, dict(mask=m), max_nprobe=mx),
                 lambda: _device(st.s, st.queries, k, nprobe, True, dict(mask=m), max_nprobe=mx)):
        for _ in range(2):
            before = st.s.counters()
            got = call()
            after = st.s.counters()
            assert after["queries"] - before["queries"] == NQ
            assert after["candidate_rows"] - before["candidate_rows"] == tot == int(np.asarray(got[3]).astype(np.int64).sum())
            assert after["embeddings_fetched"] - before["embeddings_fetched"] == cons
            runs.append(got)
    for a, b in zip(runs[0::2], runs[1::2]):
        for x, y in zip(a, b):
            assert (x is None and y is None) or (np.asarray(x).view(np.uint8) == np.asarray(y).view(np.uint8)).all()
    # a caller's stream: the copy enqueued behind the call on that stream sees the finished rows and distances
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        r_t, d_t, keep = _device(st.s, st.queries, k, nprobe, False, dict(mask=m), max_nprobe=mx, stream=stream.cuda_stream)
        r_c, d_c = r_t.clone(), d_t.clone()
    stream.synchronize()
    assert (r_c.cpu().numpy().view(np.uint32) == runs[2][0]).all() and (_bits(d_c.cpu().numpy()) == _bits(runs[2][1])).all()


def test_refusals_and_builder(shape1, pqv, oracle):
    """Case 9: the UNSUPPORTED texts, the INVALID texts that need a live handle in the contract's order, and the builder."""
    from test_gpu_table import Table
    st = shape1
    m = st.rowmasks["1/64"]
    q = st.queries

    def refused(call, code, text):
        with pytest.raises(pqv.PqvError) as e:
            call()
        assert e.value.code == code and text in str(e.value), (e.value.code, str(e.value))

    uns = "pqv_topk_expand takes k <= 1024 (1023 with tie flags) and at most 1024 probed lists per query"
    refused(lambda: st.s.topk(q, 10, 1, mask=m, max_nprobe=4, metric=pqv.PQV_DOT), -5, "PQV_DOT is not supported by pqv_topk_expand")
    refused(lambda: _device(st.s, q, 10, 1, False, dict(mask=m), max_nprobe=4, metric=pqv.PQV_DOT), -5, "PQV_DOT is not supported by pqv_topk_expand")
    refused(lambda: _device(st.s, q, 1024, 1, True, dict(mask=m), max_nprobe=4), -5, uns)
    refused(lambda: _device(st.s, q, 1025, 1, False, dict(mask=m), max_nprobe=4), -5, uns)
    refused(lambda: st.s.topk(q, 1024, 1, mask=m, max_nprobe=4), -5, uns)          # (the host form always carries tie flags)
    got = _device(st.s, q, 1024, 1, False, dict(mask=m), max_nprobe=2)             # k = 1024 without flags is served
    assert (got[5] == 2).all() and (got[2] <= 1024).all()
    t = Table(pqv, oracle, np.random.default_rng(12), [900, 1400], [4, 6], 32, gap=5)
    tm = t.s.row_mask(np.ones(len(t.data), bool))
    tq = np.zeros((2, 32), np.float32)
    refused(lambda: t.s.topk(tq, 10, 1, mask=tm, max_nprobe=2), -5, "pqv_topk_expand does not take table searchers")
    refused(lambda: _device(t.s, tq, 10, 1, False, dict(mask=tm), max_nprobe=2), -5, "pqv_topk_expand does not take table searchers")
    # INVALID, in order: max_nprobe ahead of ownership, ownership ahead of k and nprobe
    refused(lambda: st.s.topk(q, 0, 3, mask=tm, max_nprobe=2), -1, "max_nprobe must be >= nprobe")
    refused(lambda: st.s.topk(q, 0, 1, mask=tm, max_nprobe=2), -1, "row mask belongs to another searcher")
    refused(lambda: st.s.topk(q, 0, 1, mask=m, max_nprobe=2), -1, "k must be > 0")
    refused(lambda: st.s.topk(q, 10, 0, mask=m, max_nprobe=2), -1, "nprobe must be > 0")
    refused(lambda: st.s.topk(q[:, :100], 10, 1, mask=m, max_nprobe=2), -1, "Query dimension mismatch: expected 128, got 100")
    tm.close()
    # the builder: query 0 of case 1
    u0 = int(expand_ref.nprobe_used(st.oidx, st.lists, st.masks["1/64"], q[0], 10, 1, 16))
    rows, dist, nf, _ = st.s.topk(q[:1], 10, u0, mask=m)
    res = pqv.TopkBuilder(st.s, q[0]).k(10).nprobe(1).where(m).max_nprobe(16).search()
    assert [r.row_idx for r in res] == rows[0, :int(nf[0])].tolist()
    assert (_bits([r.distance for r in res]) == _bits(dist[0, :int(nf[0])])).all()
    res = pqv.TopkBuilder(st.s, q[0]).k(10).nprobe(1).where(st.masks["1/64"]).max_nprobe(16).search()      # (a bool array)
    assert [r.row_idx for r in res] == rows[0, :int(nf[0])].tolist()
