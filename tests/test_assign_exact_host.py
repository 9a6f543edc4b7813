"""tests/assign_exact.py (the f64-backed exact nearest-centroid check the full-size build tests rely on) against the C
oracle's find_closest_centroids(row, 1): the reference's chain, strict '<', lowest index wins a tie.  The data is chosen
where the f64 shortcut could go wrong: exact ties, duplicated centroids, data far from the origin (the f64 expansion
cancels), subnormal squares, non-finite values, overflowing chains and constructed near-ties whose f32 chain order
differs from exact arithmetic."""
import math

import numpy as np
import pytest

import assign_exact
from range_oracle import REF4, l2_chain

DIMS = (1, 3, 5, 768, 770)


def _oracle_nearest(oracle, X, C):
    oidx = oracle.index_from_parts(C.shape[1], C, [[] for _ in range(len(C))])
    return np.array([int(oidx.find_closest_centroids(x, 1)[0]) for x in X], dtype=np.uint32)


def _check(oracle, X, C):
    X, C = np.ascontiguousarray(X, np.float32), np.ascontiguousarray(C, np.float32)
    got, stats = assign_exact.nearest(X, C)
    want = _oracle_nearest(oracle, X, C)
    assert assign_exact.mismatches(X, C, got, want) is None, assign_exact.mismatches(X, C, got, want)
    assert stats["rows"] == len(X)
    return stats


def _near_tie(seed, dim):
    """A row and two centroids whose squared distances differ by about 1e-7 relative: the f32 chain (error up to about
    1e-5 relative at d = 768) often orders them the other way round."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(dim).astype(np.float32)
    c1 = (x + rng.standard_normal(dim).astype(np.float32)).astype(np.float32)
    c2 = c1.copy()
    idx = rng.choice(dim, size=min(dim, 4), replace=False)
    c2[idx] = (c2[idx] * (1 + rng.standard_normal(len(idx)) * 3e-7)).astype(np.float32)
    return x, np.stack([c1, c2])


# the first twelve seeds of _near_tie (per dim) whose f32 chain order differs from the exact order, found by a search
NEAR_TIE_SEEDS = {5: [17, 62, 84, 94, 112, 116, 133, 135, 137, 144, 148, 165],
                  768: [1, 3, 5, 8, 9, 11, 12, 14, 15, 16, 19, 20],
                  770: [0, 1, 6, 8, 10, 11, 13, 16, 17, 20, 21, 23]}


def _exact_order_pick(x, C):
    """Exact arithmetic: squares of f32 differences are exact in f64 and fsum rounds the sum once."""
    ex = [math.fsum(((x.astype(np.float64) - c.astype(np.float64)) ** 2).tolist()) for c in C]
    return min(range(len(C)), key=lambda j: (ex[j], j))


def _near_tie_fixture(dim):
    """Per seed: the row, then the centroids [far, c1, c2, far, far], so the pair sits in the middle of the index range."""
    rng = np.random.default_rng(dim)
    X, Cs, flips = [], [], 0
    for seed in NEAR_TIE_SEEDS[dim]:
        x, pair = _near_tie(seed, dim)
        chain = l2_chain(pair, x, REF4)
        flips += (1 if chain[1] < chain[0] else 0) != _exact_order_pick(x, pair)
        far = (x + 4 + rng.standard_normal((3, dim))).astype(np.float32)
        X.append(x)
        Cs.append(np.concatenate([far[:1], pair, far[1:]]))
    assert flips == len(NEAR_TIE_SEEDS[dim])           # every kept seed really is a near-tie the chain gets "wrong"
    return np.stack(X), Cs


@pytest.mark.parametrize("dim", DIMS)
def test_integer_data_with_exact_ties(oracle, dim):
    rng = np.random.default_rng(100 + dim)
    X = rng.integers(0, 3, size=(400, dim)).astype(np.float32)
    C = rng.integers(0, 3, size=(24, dim)).astype(np.float32)
    C[7] = C[3]                                         # duplicated centroids: the lower index must win
    C[20] = C[3]
    C[11] = C[19]
    stats = _check(oracle, X, C)
    assert stats["exact_rows"] > 0                      # integer distances tie exactly: the exact path ran


@pytest.mark.parametrize("dim", DIMS)
def test_uniform_data(oracle, dim):
    rng = np.random.default_rng(200 + dim)
    X = (rng.integers(0, 1 << 24, size=(600, dim)) * 2.0 ** -24).astype(np.float32)
    C = (rng.integers(0, 1 << 24, size=(48, dim)) * 2.0 ** -24).astype(np.float32)
    C[:8] = X[:8]                                       # centroids that are rows (distance exactly 0)
    _check(oracle, X, C)


@pytest.mark.parametrize("dim", DIMS)
def test_far_from_origin(oracle, dim):
    """Rows and centroids around -1000 with a spread of 0.01: ||x||^2 + ||c||^2 - 2 x.c cancels almost completely."""
    rng = np.random.default_rng(300 + dim)
    X = (-1000 + 0.01 * rng.standard_normal((400, dim))).astype(np.float32)
    C = (-1000 + 0.01 * rng.standard_normal((32, dim))).astype(np.float32)
    C[5] = C[9]
    _check(oracle, X, C)


@pytest.mark.parametrize("dim", DIMS)
def test_subnormal_squares(oracle, dim):
    """Differences around 1e-20 and 1e-23: their squares are subnormal or flush below the smallest subnormal."""
    rng = np.random.default_rng(400 + dim)
    X = (rng.standard_normal((300, dim)) * 1e-20).astype(np.float32)
    C = (rng.standard_normal((16, dim)) * 1e-20).astype(np.float32)
    X[::3] *= np.float32(1e-3)
    C[3] = 0.0
    C[4] = np.float32(1e-45)                            # the smallest subnormal
    stats = _check(oracle, X, C)
    assert stats["rows"] == 300


@pytest.mark.parametrize("dim", DIMS)
def test_non_finite_and_overflowing_rows(oracle, dim):
    rng = np.random.default_rng(500 + dim)
    X = rng.standard_normal((60, dim)).astype(np.float32)
    C = rng.standard_normal((12, dim)).astype(np.float32)
    X[1, 0] = np.nan
    X[2, -1] = np.inf
    X[3, 0] = -np.inf
    X[4] = np.float32(1e19)                             # squares overflow: every chain is +inf, index 0 wins
    X[5, :1] = np.float32(3e19)                         # one square overflows
    X[6] = np.float32(1e18)                             # near overflow: chains around 1e36 * dim
    C[2, 0] = np.nan                                    # a centroid that never wins
    C[6, -1] = np.inf
    stats = _check(oracle, X, C)
    assert stats["exact_rows"] >= 5


@pytest.mark.parametrize("dim", (5, 768, 770))
def test_constructed_near_ties(oracle, dim):
    X, Cs = _near_tie_fixture(dim)
    for x, C in zip(X, Cs):
        got, stats = assign_exact.nearest(x[None, :], C)
        want = _oracle_nearest(oracle, x[None, :], C)
        assert got[0] == want[0] and want[0] in (1, 2)
        assert stats["exact_rows"] == 1 and stats["max_candidates"] == 2


@pytest.mark.parametrize("dim", (5, 768, 770))
def test_negative_control_without_the_bound(oracle, dim):
    """With the bound forced to 0 the f64 estimate alone decides, and on these near-ties it picks the exactly nearest
    centroid, not the reference's: the checker disagrees with the oracle.  So the fixture exercises the exact path."""
    X, Cs = _near_tie_fixture(dim)
    wrong = 0
    for x, C in zip(X, Cs):
        got, stats = assign_exact.nearest(x[None, :], C, bound_scale=0.0)
        wrong += int(got[0] != _oracle_nearest(oracle, x[None, :], C)[0])
    assert wrong >= 1


def test_many_rows_one_near_tie_centroid_set(oracle, monkeypatch):
    """Many rows over many slabs and exact-path batches: near-tie rows scattered through uniform rows."""
    monkeypatch.setattr(assign_exact, "_slab_rows", lambda k: 257)
    monkeypatch.setattr(assign_exact, "_PAIR_BATCH", 5)
    dim = 768
    rng = np.random.default_rng(9)
    X = (rng.integers(0, 1 << 24, size=(3000, dim)) * 2.0 ** -24).astype(np.float32)
    C = (rng.integers(0, 1 << 24, size=(40, dim)) * 2.0 ** -24).astype(np.float32)
    for i, seed in enumerate(NEAR_TIE_SEEDS[768][:6]):
        x, pair = _near_tie(seed, dim)
        C[2 * i + 10:2 * i + 12] = pair
        X[500 * i + 7] = x
    stats = _check(oracle, X, C)
    assert stats["exact_rows"] >= 6


@pytest.mark.parametrize("dim", (3, 768))
def test_sensitivity_a_row_moved_to_its_second_nearest_is_reported(oracle, dim):
    rng = np.random.default_rng(700 + dim)
    X = rng.standard_normal((500, dim)).astype(np.float32)
    C = rng.standard_normal((20, dim)).astype(np.float32)
    want, _ = assign_exact.nearest(X, C)
    assert np.array_equal(want, _oracle_nearest(oracle, X, C))
    r = 321
    d2 = l2_chain(C, X[r], REF4)
    second = int(np.lexsort((np.arange(len(C)), d2))[1])
    moved = want.copy()
    moved[r] = second
    rep = assign_exact.mismatches(X, C, moved, want)
    assert rep is not None and rep["n_differ"] == 1
    f = rep["first"]
    assert (f["row"], f["got"], f["want"]) == (r, second, int(want[r]))
    assert f["chain_got"] >= f["chain_want"] and f["f64_margin"] > 0


def test_chain_gamma_and_slab_size():
    # m = 192 + 0 + 6 at d = 768: about 1.2e-5 relative, as the module docstring says
    assert 1.17e-5 < assign_exact.chain_gamma(768) < 1.19e-5
    assert assign_exact.chain_gamma(770) > assign_exact.chain_gamma(768)
    assert assign_exact._slab_rows(1024) * 1024 * 8 <= 1 << 27


def test_build_reference_accepts_the_oracle_build_and_reports_every_stage(oracle):
    """tests/build_reference.py (what the full-size GPU build tests run) on an oracle build of its own: no problem;
    a row moved to another list, or one centroid bit flipped, is reported at the stage where it happened."""
    from build_reference import check_build_against_reference, reference_blob
    n, dim, k, workers = 4000, 8, 12, 3
    rng = np.random.default_rng(21)
    data = rng.random((n, dim), dtype=np.float32)
    data[::5] += np.float32(1.5)
    oidx = oracle.build_index(data, n_clusters=k, max_iters=20, seed=42, workers=workers)
    sample_idx, _ = oracle.index_sample(oracle.rng(42), n, max(n // 20, k))     # index.rs:172-174: 200 of 4000
    blob, cent, off, rows = oidx.to_bytes(), oidx.centroids, oidx.list_off, oidx.list_rows
    problems, rec = check_build_against_reference(oracle, data, blob, cent, off, rows, sample_idx, k, workers)
    assert problems == [] and rec["n"] == n
    of = np.empty(n, np.uint32)
    of[rows] = np.repeat(np.arange(k, dtype=np.uint32), np.diff(off.astype(np.int64)))
    assert reference_blob(dim, cent, of, k)[0] == blob

    lists = [l.tolist() for l in oidx.lists()]
    r = lists[3][len(lists[3]) // 2]
    lists[3].remove(r)
    lists[5] = sorted(lists[5] + [r])
    moved = oracle.index_from_parts(dim, cent, lists)
    problems, _ = check_build_against_reference(oracle, data, moved.to_bytes(), cent, moved.list_off, moved.list_rows,
                                                sample_idx, k, workers)
    stages = {key for p in problems for key in p}
    assert {"final_assignment", "list_offsets_differ_first_at", "list_rows_differ_first_at", "blob_differs"} <= stages
    fa = next(p["final_assignment"] for p in problems if "final_assignment" in p)
    assert fa["n_differ"] == 1 and (fa["first"]["row"], fa["first"]["got"], fa["first"]["want"]) == (r, 5, 3)

    bent = cent.copy()
    bent.view(np.uint32)[7, 2] ^= 1
    problems, _ = check_build_against_reference(oracle, data, blob, bent, off, rows, sample_idx, k, workers)
    assert [list(p) for p in problems] == [["centroids_differ", "first", "max_abs_diff"]] and problems[0]["first"] == 7
