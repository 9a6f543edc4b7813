"""Multi-chunk rows without a GPU: the numpy chains the GPU module (tests/test_gpu_long_rows.py) compares against, pinned to the C
oracle bit for bit at the long dimensions; the chunk helper of tests/long_rows_cases.py against the table the kernels must see;
and the conditions on the inputs of every shape -- list lengths, pairwise distinct distances -- so that a bad seed is found here."""
import numpy as np
import pytest

import cosine_ref
import dot_ref
import long_rows_cases as L
import mask_ref
from range_oracle import REF4, SEQ, l2_chain

DIMS = [70, 96, 132, 134, 192, 260, 768]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("dim", DIMS)
def test_numpy_chains_match_the_c_oracle_bits(oracle, dim):
    """l2_chain REF4 and SEQ, dot_ref's chain (of x with itself: the oracle's chain against zero) and cosine_ref's normalisation
    (sq is the oracle's chain against zero, r and n are single float32 operations on it), mixed magnitudes per dimension."""
    rng = np.random.default_rng(dim)
    x = (rng.standard_normal((48, dim)) * rng.choice([1e-3, 1.0, 1e3], size=(1, dim))).astype(np.float32)
    q = rng.standard_normal(dim).astype(np.float32)
    zero = np.zeros(dim, np.float32)
    r4, sq, dots, csq, nx = l2_chain(x, q, REF4), l2_chain(x, q, SEQ), dot_ref.dot_chain(x, x), cosine_ref.sq(x), cosine_ref.normalise(x)
    rr = cosine_ref.r(x)
    for i in range(len(x)):
        assert _bits(r4[i]) == _bits(oracle.l2_ref4(x[i], q))
        assert _bits(sq[i]) == _bits(oracle.l2_seq(x[i], q))
        against_zero = oracle.l2_ref4(x[i], zero)
        assert _bits(dots[i]) == _bits(against_zero) and _bits(csq[i]) == _bits(against_zero)
        assert _bits(rr[i]) == _bits(np.float32(1.0) / np.sqrt(np.float32(against_zero)))
        assert (_bits(nx[i]) == _bits(x[i] * rr[i])).all()
    # one query against rows == row by row (the form Case.topk uses == the form checked above)
    assert (_bits(dot_ref.dot_chain(q, x)) == _bits(dot_ref.dot_chain(np.tile(q, (len(x), 1)), x))).all()
    # zero-padded storage changes no bit: x + 0 is x in both chains
    pad = np.zeros((len(x), 64), np.float32)
    for metric in (REF4, SEQ):
        if dim % 4 == 0:
            assert (_bits(l2_chain(np.hstack([x, pad]), np.concatenate([q, pad[0]]), metric)) == _bits(l2_chain(x, q, metric))).all()


# the issue's table: (dim, metric, row order) -> (stored dim, G, CG, chunks, tail, aligned)
TABLE = [
    (192, REF4, False, (192, 48, 32, [32, 16], 0, True)),
    (132, REF4, False, (132, 33, 32, [32, 1], 0, True)),              # no padding: 192 > 132 * 4 / 3
    (260, REF4, True, (260, 65, 32, [32, 32, 1], 0, True)),
    (260, REF4, False, (320, 80, 32, [32, 32, 16], 0, True)),
    (768, REF4, False, (768, 192, 64, [64, 64, 64], 0, True)),
    (134, REF4, False, (134, 33, 32, [32, 1], 2, False)),
    (3, REF4, False, (3, 0, 32, [], 3, False)),
    (96, SEQ, True, (96, 24, 16, [16, 8], 0, True)),
    (96, SEQ, False, (128, 32, 16, [16, 16], 0, True)),
    (70, SEQ, False, (70, 17, 16, [16, 1], 2, False)),
    # the single-chunk shapes of the older modules, for contrast
    (128, REF4, False, (128, 32, 32, [32], 0, True)),
    (256, REF4, False, (256, 64, 64, [64], 0, True)),
    (30, REF4, False, (30, 7, 32, [7], 2, False)),
    (32, SEQ, False, (32, 8, 16, [8], 0, True)),
    # the padding rule's other branches
    (200, REF4, False, (256, 64, 64, [64], 0, True)),                 # a multiple of 256 within a third
    (100, REF4, False, (128, 32, 32, [32], 0, True)),
    (52, REF4, False, (64, 16, 32, [16], 0, True)),
    (44, REF4, False, (44, 11, 32, [11], 0, True)),                   # 64 > 44 * 4 / 3: stays
]


@pytest.mark.parametrize("dim,metric,row_order,exp", TABLE)
def test_chunk_helper_restates_the_table(dim, metric, row_order, exp):
    assert L.chunk_plan(dim, metric, row_order) == exp


def test_every_shape_is_in_the_table_and_runs_the_loop_twice():
    rows = {(d, m, r): e for d, m, r, e in TABLE}
    for name, c in L.SHAPES.items():
        plan = L.plan_of(name)
        assert plan == rows[c["dim"], c["metric"], c["row_order"]], name
        sdim, g, cg, chunks, tail, aligned = plan
        assert (g, cg, chunks, tail) == c["sees"], name
        assert sum(chunks) == g and g * 4 + tail == sdim
        if c["dim"] != 3:
            assert len(chunks) >= 2, name
        else:
            assert chunks == [] and tail == 3
    # the instantiations the masked family must launch: <16, true, unaligned>, <32, false, unaligned> and <32, false, aligned> with
    # G > 32, <64, false, aligned> with G = 192
    seen = {(p[2], c["metric"] == SEQ, p[5]) for p, c in ((L.plan_of(n), L.SHAPES[n]) for n in L.L2_SHAPES) if len(p[3]) >= 2}
    assert {(16, True, False), (16, True, True), (32, False, False), (32, False, True), (64, False, True)} <= seen
    assert L.plan_of("768")[1] == 192
    assert {L.SHAPES[n]["dim"] for n in L.COS_SHAPES} == {132, 768} and {L.SHAPES[n]["dim"] for n in L.DOT_SHAPES} == {132, 134, 768}


@pytest.fixture(scope="module")
def cases(oracle):
    return {name: L.Case(name, oracle) for name in L.SHAPES}


@pytest.mark.parametrize("name", list(L.SHAPES))
def test_inputs_meet_the_conditions(cases, name):
    """Lists: one shorter than 64 rows, one longer than 512.  Distances: pairwise distinct per query over ALL rows, in the
    shape's metric; and the one sqrt_out = default top-k of the GPU module has no equal sqrt among its k + 1 nearest."""
    case = cases[name]
    case.assert_lists()
    case.assert_distinct()
    assert case.n == L.N and len(case.queries) == L.NQ and 1500 <= L.N <= 3000 and 4 <= L.KC <= 6
    for nprobe in L.NPROBES:
        assert all(len(case.cand(qi, nprobe)) == sum(len(case.lists[c]) for c in _probed(case, qi, nprobe)) for qi in range(L.NQ))
        if case.kind == "l2":
            case.topk(case.masks["1/2"], 10, nprobe, sqrt_out=True)          # (asserts inside)
        for allowed in (None if case.kind == "dot" else case.masks["1/2"], case.masks["1/64"], case.masks["1/2"]):
            assert case.radius(allowed, nprobe) == case.radius(allowed, nprobe)   # (query 0 considers a row: a radius exists)
    # every mask leaves rows to consider in the short list and in the long one
    lens = [len(l) for l in case.lists]
    short, long_ = case.lists[int(np.argmin(lens))], case.lists[int(np.argmax(lens))]
    assert case.masks["1/2"][short].any() and case.masks["1/2"][long_].sum() > 128 and case.masks["1/64"][long_].any()
    # about 16 rows per group key, a quarter of the rows per tenant, NULLs in both validity arrays
    assert 8 < L.N / len(np.unique(case.group)) < 24 and len(np.unique(case.tenant)) == 4
    assert 0 < (case.tenant_valid == 0).sum() < L.N / 2 and 0 < (case.group_valid == 0).sum() < L.N / 2


def _probed(case, qi, nprobe):
    if case.kind == "dot":
        return dot_ref.probe(case.queries[qi], case.centroids.reshape(-1, case.dim), nprobe)
    return case.oidx.find_closest_centroids(case.rq[qi], nprobe)


def test_references_agree_with_the_c_oracle_top_k(oracle, cases):
    """Case.topk (mask_ref over candidate_rows) == the C oracle's own top-k on the filtered-lists index, where the oracle has the
    call: REF4, squared distances compared after its sqrt."""
    for name in ("132", "768"):
        case = cases[name]
        allowed = case.masks["1/2"]
        f = oracle.index_from_parts(case.dim, case.centroids, mask_ref.filtered_lists(case.lists, allowed))
        for nprobe in L.NPROBES:
            rows, dist, nf, nc, tf = case.topk(allowed, 10, nprobe, sqrt_out=True)
            orows, odist, onf, _ = f.topk_batch(case.data, case.queries, 10, nprobe)
            assert (rows == orows).all() and (_bits(dist) == _bits(odist)).all() and (nf == onf).all() and not tf.any()
            assert (nc == [len(case.cand(qi, nprobe)) for qi in range(L.NQ)]).all()


def test_wide_keys_keep_order_and_words():
    v = np.arange(-3, 9)
    w = L.wide(v)
    assert w.dtype == np.int64 and (np.diff(w) > 0).all() and (w[:3] < 0).any()
    assert len(np.unique(w >> 32)) == len(v) and len(np.unique(w & 0xFFFFFFFF)) == len(v)          # both words differ between keys
