"""Every group-count-specialised K loop body of wide_filter_kernel, at the smallest shapes that reach it.

Four clusters probed by every query (nprobe = 4), so each list carries exactly `nq` pairs: up to 96 of them are ONE quad of
the regular instance with ceil(nq / 16) live groups (6 groups: the branch-free body, fewer: the generic one), 97..160 are
ONE quad of the wide-quad instance (7..10 live groups, a body each), more are a wide quad of 160 and a regular quad of the
rest.  The accumulators start from the C operand of their first MFMA and the validity words of a tile are built from
wave-uniform masks plus the quad's last group, so the cases carry the edge values of both: list lengths that are no multiple
of 32 or 64 (a partial last tile), a list shorter than the seed window, a query equal to a corpus row (distance 0), a list of
identical rows (zero residuals), query counts that end in the middle of a group and of a lane's four queries.
Row ids and distance bits must equal the CPU oracle's."""
import numpy as np
import pytest

from test_gpu_parity import _assert_topk_equal

pytestmark = pytest.mark.gpu

SIZES = [4003, 2777, 1381, 39]          # rows per cluster: 8200 in all; 1381 identical rows; 39 < the 64-row seed window
NQ_MAX = 200


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def make_case(dim):
    """Corpus, cluster of every row, queries.  The queries lie near the two large clusters only: the list of identical rows is
    screened by every query but never reaches a top-k, so no result hangs on a tie at the boundary."""
    rng = np.random.default_rng(5150 + dim)
    cen = (rng.standard_normal((len(SIZES), dim)) * 2.0).astype(np.float32)
    parts = [cen[c] + 0.3 * rng.standard_normal((m, dim)).astype(np.float32) for c, m in enumerate(SIZES)]
    parts[2][:] = cen[2]                                                        # a constant list: zero residuals
    perm = rng.permutation(sum(SIZES))
    data = np.ascontiguousarray(np.concatenate(parts)[perm].astype(np.float32))
    label = np.repeat(np.arange(len(SIZES)), SIZES)[perm]
    near = cen[rng.integers(0, 2, size=NQ_MAX)]
    queries = (near + 0.4 * rng.standard_normal((NQ_MAX, dim))).astype(np.float32)
    # a query equal to a corpus row, first and in the middle of a group (every case below has at least 17 queries)
    in_a = np.flatnonzero(label == 0)
    queries[0] = data[in_a[0]]
    queries[13] = data[in_a[1]]
    return data, label, np.ascontiguousarray(queries)


class _Case:
    def __init__(self, pqv, oracle, dim):
        self.dim = dim
        self.data, label, self.queries = make_case(dim)
        # the lists are given, not found by k-means: their lengths are the point (centres: the clusters' means)
        lists = [np.flatnonzero(label == c) for c in range(len(SIZES))]
        cent = np.stack([self.data[l].astype(np.float64).mean(axis=0) for l in lists]).astype(np.float32)
        self.oidx = oracle.index_from_parts(dim, cent, lists)
        self.index = pqv.Index.from_bytes(self.oidx.to_bytes())
        self.corpus = pqv.Corpus.upload(self.data)
        lens = np.diff(self.index.list_offsets.astype(np.int64))
        assert lens.tolist() == SIZES and (lens % 32 != 0).all() and lens.min() < 64
        self._ref = {}

    def reference(self, k, nq):
        """The oracle's answer for the first nq queries (computed once per k for all of them: queries are independent)."""
        if k not in self._ref:
            self._ref[k] = self.oidx.topk_batch(self.data, self.queries, k, len(SIZES))
        return tuple(a[:nq] for a in self._ref[k])


_cases = {}


@pytest.fixture
def case(pqv, oracle):
    def get(dim):
        if dim not in _cases:
            _cases[dim] = _Case(pqv, oracle, dim)
        return _cases[dim]
    return get


def _check(pqv, c, nq, k, op="int8", S=1, wide=None, deferred=False, defp=False, options=()):
    nprobe = len(SIZES)
    s = pqv.Searcher(c.index, c.corpus)
    s.set_option("rerank_mode", 2); s.set_option("tile_filter", 2)
    for name, value in options:
        s.set_option(name, value)
    d = s.describe(nq, k, nprobe)
    opn = {"int8": 2, "f16": 1}[op]
    assert f"{op} screen operands" in d and "quads of 96 queries" in d and "4 waves per block" in d, d
    tail = "true" if defp else "false"               # (DEFP: the deferred form compiled into a k <= 64 instance)
    nt = "true" if "lists probed by 97..160 queries" in d else "false"
    assert f"wide_filter_kernel<6, 4, {S}, true, {opn}, false, {nt}, 4, {tail}>" in d, d
    if wide is not None:
        # every list carries nq pairs: 97..160 of them are one quad of the wide-quad instance
        assert nt == "true" and f"wide_filter_kernel<10, 8, {S}, true, 2, false, " in d and f", 2, {tail}>" in d, d
    assert ("exact evaluations deferred" in d) == deferred, d
    queries = c.queries[:nq]
    orows, odist, onf, onc = c.reference(k, nq)
    assert _bits(odist[0, :1])[0] == 0 and _bits(odist[13, :1])[0] == 0          # the queries that ARE corpus rows
    for _ in range(2):                     # (twice: the second call meets the first one's scratch)
        rows, dist, nf, nc = s.topk(queries, k, nprobe)
        assert (nc == onc).all() and (nf == onf).all()
        assert (_bits(dist) == _bits(odist)).all(), (nq, k)
        _assert_topk_equal((rows, dist, nf), (orows, odist, onf), k)      # (ids position by position; as sets inside equal distances)


@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("nq", [17, 33, 49, 65, 81, 96])
def test_regular_instance_every_group_count(pqv, case, nq, k):
    """2 (the generic body), 3, 4, 5 and 6 live groups of the regular instance <6, 4>; 96 fills the quad, the others end inside a
    group's first lane quartet."""
    _check(pqv, case(256), nq, k)


@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("nq", [97, 113, 129, 145, 160])
def test_wide_quad_instance_every_group_count(pqv, case, nq, k):
    """7, 8, 9 and 10 live groups of the wide-quad instance <10, 8> (32-row tiles), a K loop body each."""
    _check(pqv, case(256), nq, k, wide=True)


@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("nq", [161, 200])
def test_several_quads_per_list(pqv, case, nq, k):
    """A wide quad of 160 and a regular quad of the rest (1 query: one live group with one live lane quartet; 40: three groups)."""
    _check(pqv, case(256), nq, k, wide=True)


@pytest.mark.parametrize("defer", [0, 1])
@pytest.mark.parametrize("dim", [512, 768])
def test_longer_rows(pqv, case, dim, defer):
    """8 and 12 K steps per tile instead of 4 (the loop behind the peeled steps runs more than once); 130 queries: 9 groups.
    Short lists of rows this long defer their exact evaluations by rule (the DEFP instances); with the rule switched off the
    instances are those of the 10 M x 768 benchmark."""
    _check(pqv, case(dim), 130, 10, wide=True, deferred=bool(defer), defp=bool(defer), options=(("defer", defer),))


def test_f16_operands(pqv, case):
    """The f16 form of the same template (float accumulators: their start value is the inline zero), a full quad of 96."""
    _check(pqv, case(128), 96, 10, op="f16")


def test_deferred_form(pqv, case):
    """k = 70: the k > 64 instances, which carry the deferred evaluation -- the accumulators are read again AFTER the screen (the
    survivors' raw scores), in both instances."""
    _check(pqv, case(256), 130, 70, S=4, wide=True, deferred=True, options=(("screen_i8", 2),))
