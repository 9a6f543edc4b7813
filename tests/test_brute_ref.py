"""Self-checks of brute_ref.py: the checker rejects answers that are subtly wrong, the slabbed reference is the unslabbed one, and
the pre-conditions the GPU tests of test_gpu_brute_forms.py rest on hold for their fixed seeds -- the cap on the rows the tolerance
leaves unchecked, and the construction that makes a row range overflow.  No GPU."""
import numpy as np
import pytest

import brute_ref as br


def _perfect(ref, k):
    """the answer an exact f32 implementation would give: the reference's rows with f32 distances, keyed like the library"""
    kk = ref.kk(k)
    rows = np.full((ref.nq, k), br.NONE, np.uint32)
    dist = np.full((ref.nq, k), np.inf, np.float32)
    d32 = ref.dist[:, :kk].astype(np.float32)
    key = (br.sortable_bits(d32).astype(np.uint64) << np.uint64(32)) | ref.order[:, :kk].astype(np.uint64)
    o = np.argsort(key, axis=1)
    rows[:, :kk] = np.take_along_axis(ref.order[:, :kk], o, axis=1)
    dist[:, :kk] = np.take_along_axis(d32, o, axis=1)
    return rows, dist, np.full(ref.nq, kk, np.uint32)


@pytest.fixture(scope="module", params=[br.COS, br.L2])
def small(request):
    data, queries = br.make_case("normal", 3000, 24, 9)
    return br.reference(data, queries, 40, request.param)


def test_checker_accepts_the_exact_answer(small):
    for k in (1, 10, 40):
        br.check(small, k, *_perfect(small, k))
    few = br.reference(small.data[:7], small.queries, 10, small.metric)          # k > n
    br.check(few, 10, *_perfect(few, 10))


@pytest.mark.parametrize("defect", ["dropped", "swapped", "twice", "distance", "found", "tail", "far row"])
def test_checker_rejects_a_wrong_answer(small, defect):
    k = 10
    rows, dist, nf = _perfect(small, k)
    if defect == "dropped":            # the nearest row is missing, the 11th takes the last place
        rows[4, :-1], dist[4, :-1] = rows[4, 1:].copy(), dist[4, 1:].copy()
        rows[4, -1], dist[4, -1] = small.order[4, 10], np.float32(small.dist[4, 10])
    elif defect == "swapped":
        rows[2, [3, 4]], dist[2, [3, 4]] = rows[2, [4, 3]], dist[2, [4, 3]]
    elif defect == "twice":
        rows[6, 5], dist[6, 5] = rows[6, 4], dist[6, 4]
    elif defect == "distance":
        dist[1, 0] *= np.float32(1.0 - 3e-4) if small.metric == br.COS else np.float32(1.0 - 2e-3)
    elif defect == "found":
        nf[3] = k - 1
    elif defect == "tail":
        rows, dist, nf = _perfect(br.reference(small.data[:7], small.queries, k, small.metric), k)
        rows[0, 8] = 3
    elif defect == "far row":          # a row from far outside the top k in the last place, with a distance that keeps the order
        rows[5, -1] = small.order[5, 39]
    ref = br.reference(small.data[:7], small.queries, k, small.metric) if defect == "tail" else small
    with pytest.raises(AssertionError):
        br.check(ref, k, rows, dist, nf)


def test_checker_refuses_a_case_its_tolerance_would_hide():
    """twelve copies of one row: all of the top 10 tie with the k-th, so nothing could be checked"""
    data, queries = br.make_case("normal", 3000, 24, 4)
    data[500:512] = queries[0] * np.float32(1.5)
    ref = br.reference(data, queries, 10, br.COS)
    assert ref.left_out(10)[0] == 10
    with pytest.raises(AssertionError, match="unchecked"):
        br.check(ref, 10, *_perfect(ref, 10))


def test_slabs_do_not_change_the_reference(small):
    again = br.reference(small.data, small.queries, 40, small.metric, slab=4)
    assert np.array_equal(again.order, small.order) and np.allclose(again.dist, small.dist, rtol=1e-13, atol=0)    # (BLAS blocks the products differently)
    sub = small.take(slice(2, 5))
    assert np.array_equal(sub.order, small.order[2:5]) and sub.nq == 3


def test_order_contract_uses_the_library_key():
    d = np.array([-1.0, -0.0, 0.0, 1e-30, 1.0, np.inf], np.float32)
    b = br.sortable_bits(d)
    assert (np.diff(b.astype(np.int64)) > 0).all()
    assert np.array_equal(b[2:] ^ np.uint32(0x80000000), d[2:].view(np.uint32))   # non-negative: the uint32 view orders the same


@pytest.mark.parametrize("kind,dim", br.FORM_CASES, ids=[f"{k}-{d}" for k, d in br.FORM_CASES])
def test_cap_holds_for_the_form_cases(kind, dim):
    data, queries = br.make_case(kind, br.N_FORMS, dim, 130)
    for metric in (br.COS, br.L2):
        br.reference(data, queries, 10, metric).assert_cap(10)


def test_cap_holds_for_the_shape_edge_cases():
    data, queries = br.make_case("normal", br.N_FORMS, 64, 257)
    for metric in (br.COS, br.L2):
        ref = br.reference(data, queries, 1024, metric)
        for k in (1, 10, 64, 65, 256, 257, 1024):
            ref.assert_cap(k)


def test_hostile_case_holds_what_it_promises():
    data, queries = br.make_case("hostile", br.N_FORMS, 160, 130)
    norms = np.linalg.norm(data.astype(np.float64), axis=1)
    assert (norms == 0).sum() == 3 and norms[norms > 0].min() < 1e-10 and norms.max() > 1e13
    for metric in (br.COS, br.L2):
        ref = br.reference(data, queries, 10, metric)
        first = br.NEAR_FIRST + br.NEAR_PER_QUERY * np.arange(130)
        assert np.array_equal(ref.order[:, 0], first)                   # the top 10 of every query are its own near-duplicates,
        assert ((ref.order >= first[:, None]) & (ref.order < first[:, None] + br.NEAR_PER_QUERY)).all()      # beyond row 18 432


@pytest.mark.parametrize("metric", [br.COS, br.L2])
@pytest.mark.parametrize("n", [30_000, 36_000])
def test_sorted_rows_overflow_their_ranges(n, metric):
    data, queries = br.make_sorted_towards_queries(n, 64, 130)
    assert np.allclose(np.linalg.norm(data.astype(np.float64), axis=1), 1.0, atol=1e-6)
    br.assert_ranges_overflow(data, queries, 10, metric, 2048, 18432)
    br.assert_ranges_overflow(data, queries, 10, metric, 8192, n)
    if n >= 32768:
        br.assert_ranges_overflow(data, queries, 10, metric, 18432, n)
    br.reference(data, queries, 10, metric).assert_cap(10)
    with pytest.raises(AssertionError):                                  # (the check can fail: the same rows sorted AWAY from the queries)
        br.assert_ranges_overflow(data[::-1].copy(), queries, 10, metric, 2048, 18432)
