"""The int8 screen instances with the row length compiled in (wide_filter_kernel<..., DIM = 768>), where they actually run.

Only the LDS addresses of the A-operand reads differ from the run-time form (four lane addresses plus immediates, K loops
unrolled), so every answer must stay what it was, bit for bit.  Corpus: 10 000 x 768 uniform f32 in 16 clusters (about 625 rows
per list, none a multiple of the 64-row tile), k = 10.  Each case asserts that the dispatch text names the instances and the
form, that row ids and distance bits equal the CPU oracle's, and that row ids, distance bits and candidate counts equal the same
searcher's with static_dim = 0.

  wide-quad instance   256 queries, nprobe 8: about 128 pairs per list -- lists in the 97..160 band (one wide quad) and above 160
                       (a wide quad and a regular one)
  regular instance     nprobe 4 with 16, 64, 150 and 350 queries: about 4, 16, 37 and 87 pairs per list (one to six live groups);
                       350 queries once more with wide_quads = 0, where the lists above 96 pairs are cut into full 96-pair quads
  k = 1, k = 16        once each
  run-time form        a 512-dim corpus of the same size: no instance has that length compiled in, the text says so
  mutated indexes      an appended index and a removed-and-compacted one (lists that end inside a 64-row tile at other places)"""
import numpy as np
import pytest

from test_gpu_parity import _assert_topk_equal

pytestmark = pytest.mark.gpu

N, KC, NQ_MAX = 10000, 16, 350
COMPILED = "row length compiled in (768 dims"
RUNTIME = "row length read at run time"
REGULAR = "wide_filter_kernel<6, 4, 1, true, 2, false, "
WIDE = "wide_filter_kernel<10, 8, 1, true, 2, false, "


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class _Case:
    """A corpus, an index over it (the library's, re-read by the oracle from its blob) and the oracle's answers, made once."""

    def __init__(self, pqv, oracle, dim, state="built"):
        rng = np.random.default_rng(768000 + dim + {"built": 0, "appended": 1, "compacted": 2}[state])
        X = rng.random((N, dim), dtype=np.float32)
        self.queries = rng.random((NQ_MAX, dim), dtype=np.float32)
        if state == "built":
            self.corpus = pqv.Corpus.upload(X)
            self.index = pqv.IndexBuilder(self.corpus).n_clusters(KC).max_iters(5).workers(1).build()
        else:
            n0 = 8000
            corpus = pqv.Corpus.create(N, dim)
            corpus.append(X[:n0])
            index = pqv.IndexBuilder(corpus).n_clusters(KC).max_iters(5).workers(1).build()
            corpus.append(X[n0:])
            index = index.append(corpus)
            if state == "compacted":
                index = index.remove(flags=rng.random(N) < 0.35)
                corpus, index, old_row = index.compact(corpus)
                X = X[old_row.astype(np.int64)]
            self.corpus, self.index = corpus, index
        self.data = np.ascontiguousarray(X)
        self.oidx = oracle.index_from_bytes(self.index.to_bytes())
        lens = np.diff(self.index.list_offsets.astype(np.int64))
        assert lens.sum() == len(self.data) and (lens % 64 != 0).any()
        self._ref = {}

    def reference(self, k, nprobe, nq):
        if (k, nprobe) not in self._ref:
            self._ref[(k, nprobe)] = self.oidx.topk_batch(self.data, self.queries, k, nprobe)
        return tuple(a[:nq] for a in self._ref[(k, nprobe)])


_cases = {}


@pytest.fixture
def case(pqv, oracle):
    def get(dim=768, state="built"):
        if (dim, state) not in _cases:
            _cases[(dim, state)] = _Case(pqv, oracle, dim, state)
        return _cases[(dim, state)]
    return get


def _check(pqv, c, nq, nprobe, k=10, wide=None, compiled=True, options=()):
    """wide: the wide-quad instance is part of the dispatch (True: wide_quads = 2, which does not look at the previous batch's
    shape) or is not (False); None: the default rule, whatever it says for each call"""
    s = pqv.Searcher(c.index, c.corpus)
    # (the wide int8 screen for every batch size, exact evaluation in the kernel: the instances of the 10 M x 768 benchmark)
    # (96-query quads whatever the pair count per list: the rule takes the 64-query instance for small batches)
    s.set_option("rerank_mode", 2); s.set_option("tile_filter", 2); s.set_option("defer", 0); s.set_option("quad_width", 96)
    for name, value in tuple(options) + ((("wide_quads", 2),) if wide else ()):
        s.set_option(name, value)
    d = s.describe(nq, k, nprobe)
    assert "int8 screen operands" in d and "quads of 96 queries" in d and REGULAR in d, d
    assert wide is None or (WIDE in d) == wide, d
    assert ((COMPILED if compiled else RUNTIME) in d) and ((RUNTIME if compiled else COMPILED) not in d), d
    queries = c.queries[:nq]
    orows, odist, onf, onc = c.reference(k, nprobe, nq)
    rows, dist, nf, nc = s.topk(queries, k, nprobe)
    assert (nc == onc).all() and (nf == onf).all()
    assert (_bits(dist) == _bits(odist)).all(), (nq, k)
    _assert_topk_equal((rows, dist, nf), (orows, odist, onf), k)
    # the same searcher on the run-time form
    s.set_option("static_dim", 0)
    d0 = s.describe(nq, k, nprobe)
    assert RUNTIME in d0 and COMPILED not in d0 and REGULAR in d0 and (wide is None or (WIDE in d0) == wide), d0
    rows0, dist0, nf0, nc0 = s.topk(queries, k, nprobe)
    assert (rows == rows0).all() and (_bits(dist) == _bits(dist0)).all() and (nf == nf0).all() and (nc == nc0).all()


def test_wide_quad_instance(pqv, case):
    """About 128 pairs per list: one wide quad of 97..160 pairs on most lists, a wide quad and a regular one above 160."""
    _check(pqv, case(), 256, 8, wide=True)


@pytest.mark.parametrize("nq", [16, 64, 150, 350])
def test_regular_instance_group_counts(pqv, case, nq):
    """About 4, 16, 37 and 87 pairs per list: one to six live groups of a regular quad (350: some lists pass 96 pairs)."""
    _check(pqv, case(), nq, 4)


def test_regular_instance_full_quads(pqv, case):
    """No wide quads: a list of more than 96 pairs is a FULL regular quad (the branch-free body) and a second one of the rest."""
    _check(pqv, case(), 350, 4, wide=False, options=(("wide_quads", 0),))


@pytest.mark.parametrize("k", [1, 16])
def test_other_k(pqv, case, k):
    _check(pqv, case(), 64, 4, k=k)


def test_run_time_form_elsewhere(pqv, case):
    """512 dims: the same two instances, the row length a kernel argument (no 512-dim instance has it compiled in)."""
    _check(pqv, case(512), 256, 8, wide=True, compiled=False)


@pytest.mark.parametrize("state", ["appended", "compacted"])
def test_mutated_index(pqv, case, state):
    """Lists grown by an append, and thinned by a remove and renumbered by a compact: other lengths, other partial last tiles."""
    c = case(768, state)
    _check(pqv, c, 150, 4)
    _check(pqv, c, 256, 8, wide=True)
