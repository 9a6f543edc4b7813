"""An f64 reference of pqv_brute_topk (cosine / squared L2), the project's acceptance rule for a top-k answer, and the corpora the
brute-force tests run on.  numpy only: no GPU, and nothing of the library is imported.

The rule (tests/test_gpu_parity.py, test_brute_mfma_matches_f64_oracle and test_brute_screen_on_hostile_data):
  * every returned distance is within  1e-4 max(|d|, 1e-3) + 1e-6  of the reference's distance at the same rank; squared L2 adds
    4e-6 (|q|^2 + |v|^2), the cancellation error of the norm expansion |q|^2 + |v|^2 - 2 q.v in f32;
  * the TRUE (f64) distance of every returned row is within that tolerance of the reference's k-th distance;
  * every reference row clearly inside the k-th place (further than the tolerance below it) is returned;
  * the answer is ordered by the key the library selects with: (sortable bits of the f32 distance, row id), strictly ascending --
    for the non-negative distances of every case here that is the uint32 view of the distance.
The tolerance cannot hide a failure: per query at most  3 + k / 20  of the k reference rows (the k-th included) may lie within the
tolerance of the k-th distance and so escape the membership check.  `check` asserts that from the reference alone, before it
looks at the answer under test."""
import numpy as np

COS, L2 = "cos", "l2"
NONE = 0xFFFFFFFF


def sortable_bits(d):
    """device_common.hpp: sortable_bits -- a uint32 that orders like the float (negative values included)"""
    b = np.ascontiguousarray(d, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def _norms2(x):
    return np.einsum("ij,ij->i", x, x)


def _slab_distances(d64, v2, q64, metric):
    s = q64 @ d64.T
    q2 = _norms2(q64)
    if metric == COS:
        with np.errstate(divide="ignore", invalid="ignore"):
            dist = 1.0 - s / np.sqrt(q2[:, None] * v2[None, :])
        dist[~np.isfinite(dist)] = 1.0                 # a zero vector: distance 1 by definition
        return dist
    return q2[:, None] + v2[None, :] - 2.0 * s


def pair_distances(data, queries, rows, metric):
    """f64 distance of query q to each of rows[q] (rows: [nq, m] indices into data)"""
    q64 = np.asarray(queries, np.float64)
    out = np.empty(rows.shape, np.float64)
    for q in range(len(q64)):
        v = np.asarray(data[rows[q]], np.float64)
        out[q] = _slab_distances(v, _norms2(v), q64[q:q + 1], metric)[0]
    return out


class Reference:
    """The kmax nearest rows of every query in f64: order [nq, kmax] (ties by row id), dist [nq, kmax]; q2 [nq], v2 [n]."""

    def __init__(self, data, queries, metric, order, dist, q2, v2):
        self.data, self.queries, self.metric = data, queries, metric
        self.order, self.dist, self.q2, self.v2 = order, dist, q2, v2
        self.n, self.nq, self.kmax = len(data), len(queries), order.shape[1]

    def kk(self, k):
        assert min(k, self.n) <= self.kmax, "reference was computed for a smaller k"
        return min(k, self.n)

    def cancel(self, k):
        """[nq, kk]: the L2 cancellation term of each reference pair (0 for cosine)"""
        kk = self.kk(k)
        if self.metric != L2:
            return np.zeros((self.nq, kk))
        return 4e-6 * (self.q2[:, None] + self.v2[self.order[:, :kk]])

    def tol_kth(self, k):
        """[nq]: the tolerance at the k-th place"""
        kk = self.kk(k)
        kth = self.dist[:, kk - 1]
        t = 1e-4 * np.maximum(np.abs(kth), 1e-3) + 1e-6
        if self.metric == L2:
            t = t + 4e-6 * (self.q2 + self.v2[self.order[:, :kk]].max(axis=1))
        return t

    def left_out(self, k):
        """[nq]: how many of the k reference rows are within the tolerance of the k-th distance (the k-th itself included)"""
        kk = self.kk(k)
        return (self.dist[:, :kk] >= (self.dist[:, kk - 1] - self.tol_kth(k))[:, None]).sum(axis=1)

    def assert_cap(self, k):
        lo = self.left_out(k)
        cap = 3 + k / 20
        assert (lo <= cap).all(), f"the tolerance leaves {int(lo.max())} of {k} rows unchecked (query {int(lo.argmax())}): more than {cap}"

    def take(self, sel):
        """the reference of a subset of the queries"""
        return Reference(self.data, self.queries[sel], self.metric, self.order[sel], self.dist[sel], self.q2[sel], self.v2)


def reference(data, queries, kmax, metric, slab=256):
    """f64 top-kmax of every query, computed in slabs of `slab` queries (an [slab, n] f64 matrix at a time)."""
    assert metric in (COS, L2)
    d64 = np.asarray(data, np.float64)
    q64 = np.asarray(queries, np.float64).reshape(-1, d64.shape[1])
    v2 = _norms2(d64)
    n, kk = len(d64), min(kmax, len(d64))
    order = np.empty((len(q64), kk), np.int64)
    dist = np.empty((len(q64), kk), np.float64)
    for q0 in range(0, len(q64), slab):
        full = _slab_distances(d64, v2, q64[q0:q0 + slab], metric)
        part = np.argpartition(full, kk - 1, axis=1)[:, :kk] if kk < n else np.tile(np.arange(n), (len(full), 1))
        part.sort(axis=1)                                                  # row ids ascending, so the stable sort breaks ties by row
        d = np.take_along_axis(full, part, axis=1)
        o = np.argsort(d, axis=1, kind="stable")
        order[q0:q0 + slab] = np.take_along_axis(part, o, axis=1)
        dist[q0:q0 + slab] = np.take_along_axis(d, o, axis=1)
    return Reference(data, np.asarray(queries).reshape(-1, d64.shape[1]), metric, order, dist, _norms2(q64), v2)


def check_order(rows, dist, nf, n, k):
    """The order contract alone, for every query: nf = min(k, n) results, (distance bits, row) strictly ascending -- hence unique
    rows --, valid row ids, the unused tail filled with 0xFFFFFFFF / +inf."""
    kk = min(k, n)
    assert rows.shape == dist.shape and rows.shape[1] == k
    assert (nf == kk).all(), "n_found"
    assert (rows[:, :kk] < n).all(), "row id out of range"
    assert (rows[:, kk:] == NONE).all() and np.isposinf(dist[:, kk:]).all(), "unused tail"
    key = (sortable_bits(dist[:, :kk]).astype(np.uint64) << np.uint64(32)) | rows[:, :kk].astype(np.uint64)
    assert (key[:, 1:] > key[:, :-1]).all(), "keys not strictly ascending"
    srt = np.sort(rows[:, :kk], axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), "a row returned twice"


def check(ref, k, rows, dist, nf, what=""):
    """The whole rule for one answer (rows [nq, k] uint32, dist [nq, k] f32, nf [nq]) against `ref`."""
    ref.assert_cap(k)                                  # from the reference alone, before the answer is looked at
    kk = ref.kk(k)
    check_order(rows, dist, nf, ref.n, k)
    odist = ref.dist[:, :kk]
    tol = 1e-4 * np.maximum(np.abs(odist), 1e-3) + 1e-6 + ref.cancel(k)
    err = np.abs(dist[:, :kk].astype(np.float64) - odist)
    assert (err <= tol).all(), f"{what}: distance off by {err.max():.3e} at {np.unravel_index((err - tol).argmax(), err.shape)}"
    tk = ref.tol_kth(k)
    true = pair_distances(ref.data, ref.queries, rows[:, :kk].astype(np.int64), ref.metric)
    bad = true > (odist[:, -1] + tk)[:, None]
    assert not bad.any(), f"{what}: query {int(bad.any(axis=1).argmax())} returns a row beyond the k-th place"
    sure = odist < (odist[:, -1] - tk)[:, None]
    for q in range(ref.nq):
        miss = np.setdiff1d(ref.order[q, :kk][sure[q]], rows[q, :kk])
        assert miss.size == 0, f"{what}: query {q} misses rows {miss[:8].tolist()} that are clearly inside the top {k}"


def assert_same_bits(a, b, what=""):
    """two answers (rows, dist, nf): identical rows and identical distance bits"""
    assert np.array_equal(a[0], b[0]), f"{what}: rows differ at {np.argwhere(a[0] != b[0])[:4].tolist()}"
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), f"{what}: distance bits differ"
    assert np.array_equal(a[2], b[2]), f"{what}: n_found differs"


# ---------------------------------------------------------------------------------------
# corpora
# ---------------------------------------------------------------------------------------
N_FORMS = 35_001            # [0, 2048) [2048, 18432) [18432, 35001): the last range is 64 full 256-row tiles + 185 rows
NEAR_FIRST, NEAR_PER_QUERY = 24_000, 12
FORM_CASES = [("normal", d) for d in (7, 32, 50, 64, 96, 100, 160, 256, 1536)] + \
             [("uniform01", 96), ("uniform01", 256), ("hostile", 160), ("hostile", 256)]


def make_case(kind, n, dim, nq, seed=None):
    """(data [n, dim] f32, queries [nq, dim] f32).  Every corpus holds a zero row in the exact first range and one in a screened range."""
    rng = np.random.default_rng(n + dim if seed is None else seed)
    if kind == "normal":
        data = rng.standard_normal((n, dim)).astype(np.float32)
        queries = rng.standard_normal((nq, dim)).astype(np.float32)
    elif kind == "uniform01":                          # the bench's one-sided data: what the int8 image's mid-range term is for
        data = rng.random((n, dim), dtype=np.float32)
        queries = rng.random((nq, dim), dtype=np.float32)
    elif kind == "hostile":
        return _hostile(rng, n, dim, nq)
    else:
        raise ValueError(kind)
    data[123] = 0
    if n > 20_000:
        data[20_000] = 0
    return data, queries


def _hostile(rng, n, dim, nq):
    """test_brute_screen_on_hostile_data's ingredients at n >= 26 000: rows with one dominant component (a coarse int8 grid for the
    rest), norms scaled by 1e-12 and 1e12, zero rows, a query with a dominant component, and NEAR_PER_QUERY near-duplicates of
    every query beyond row 18 432, their noise growing by half from one to the next (so no two of them tie within the tolerance)."""
    assert n >= NEAR_FIRST + NEAR_PER_QUERY * nq and dim >= 12
    data = rng.standard_normal((n, dim)).astype(np.float32)
    queries = rng.standard_normal((nq, dim)).astype(np.float32)
    queries[3, 11] += 80.0
    for lo in (5_000, 20_000):
        data[lo:lo + 200, 7] += 60.0
        data[lo + 1_000:lo + 1_100] *= np.float32(1e-12)
        data[lo + 2_000:lo + 2_100] *= np.float32(1e12)
        data[lo + 3_000] = 0
    data[123] = 0
    sigma = (0.02 * 1.5 ** np.arange(NEAR_PER_QUERY)).astype(np.float32)
    for q in range(nq):
        lo = NEAR_FIRST + NEAR_PER_QUERY * q
        data[lo:lo + NEAR_PER_QUERY] = queries[q] + sigma[:, None] * rng.standard_normal((NEAR_PER_QUERY, dim)).astype(np.float32)
    return data, queries


SORTED_BOUNDS = ((0, 2048, 1.20, 1.15), (2048, 8192, 1.05, 0.95), (8192, None, 0.85, 0.20))


def make_sorted_towards_queries(n, dim, nq, seed=None):
    """Unit rows cos(t_i) u + sin(t_i) w_i with w_i orthogonal to u and the angle t_i falling with the row index, in three runs with
    gaps between them (SORTED_BOUNDS); queries u + noise of norm 0.01, times a positive scale.  Every row is nearer to every query
    than all rows before it, so each new row range beats the thresholds so far with all of its rows.
    Two choices keep the tolerance from hiding the top k (Reference.assert_cap): the noise lies in an 8-dimensional subspace that
    every w_i is orthogonal to, so a query's distances fall with t_i exactly instead of with a jitter of 0.01 sin(t) / sqrt(dim) on
    top; and inside a run the angle falls like the square root of the rows left, so the last rows are 1e-4 and more apart in
    distance where an even spacing would put several of them inside the L2 tolerance."""
    rng = np.random.default_rng(n + dim if seed is None else seed)
    basis, _ = np.linalg.qr(rng.standard_normal((dim, 9)))          # column 0: u; columns 1-8: the noise subspace
    u = basis[:, 0]
    w = rng.standard_normal((n, dim))
    w -= (w @ basis) @ basis.T
    w /= np.linalg.norm(w, axis=1)[:, None]
    theta = np.empty(n)
    for lo, hi, t0, t1 in SORTED_BOUNDS:
        hi = n if hi is None else hi
        theta[lo:hi] = t1 + (t0 - t1) * np.sqrt(np.linspace(1.0, 0.0, hi - lo))
    data = (np.cos(theta)[:, None] * u[None, :] + np.sin(theta)[:, None] * w).astype(np.float32)
    noise = rng.standard_normal((nq, 8)) @ basis[:, 1:].T
    noise *= 0.01 / np.linalg.norm(noise, axis=1)[:, None]
    queries = ((u[None, :] + noise) * rng.uniform(0.5, 2.0, (nq, 1))).astype(np.float32)
    return data, queries


def assert_ranges_overflow(data, queries, k, metric, first, second_end):
    """The split pre-condition, from f64 alone: for every query EVERY row of [first, second_end) is nearer than the k-th nearest row
    of [0, first), by more than the tolerance there -- so a range [first, second_end) appends all of its rows."""
    head = reference(data[:first], queries, k, metric)
    d64, q64 = np.asarray(data[first:second_end], np.float64), np.asarray(queries, np.float64)
    worst = _slab_distances(d64, _norms2(d64), q64, metric).max(axis=1)
    assert (worst < head.dist[:, k - 1] - head.tol_kth(k)).all(), "rows that do not beat the first range's k-th place"
