"""Index remove and compact on the GPU (pqv_index_remove / _device / _rows, pqv_index_compact).  Every expectation comes from code
that is not under test: the lists from the numpy model tests/remove_ref.py, the blobs from the oracle's index_from_parts, the
searches from the oracle's top-k over the model's lists.  Shapes: the oracle-built lists of test_gpu_append.py, a hand-made index
(empty lists first, last and adjacent; 63 / 64 / 65 rows; one list longer than a block's share of positions; ids not sorted
across lists) and a 16-cluster index whose lists stay above plan_topk's 192-row rule after half of the rows left."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import append_ref
import assign_exact
import remove_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"d30_k7": (30, 7, 3000), "d72_k128": (72, 128, 5000)}          # name -> (dim, k, n), lists from the oracle's build
CASES = ["d30_k7", "d72_k128", "hand_made"]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Case:
    def __init__(self, pqv, oracle, name):
        if name == "hand_made":
            self.dim, self.C, self.lists = remove_ref.hand_made(dim=64)
            self.k = len(self.lists)
            self.n = sum(remove_ref.LENGTHS) + remove_ref.HAND_MADE_SPARE
            self.X = np.random.default_rng(64).random((self.n, self.dim), dtype=np.float32)
            self.index = pqv.Index.from_parts(self.dim, self.C, self.lists)
        else:
            self.dim, self.k, self.n = SHAPES[name]
            self.X = np.random.default_rng(self.dim).random((self.n, self.dim), dtype=np.float32)
            oidx = oracle.build_index(self.X, n_clusters=self.k, max_iters=5, workers=1)
            self.C, self.lists = oidx.centroids, oidx.lists()
            self.index = pqv.Index.from_bytes(oidx.to_bytes())
        self.blob = self.index.to_bytes()
        self.bound = append_ref.row_bound(self.lists)
        self.patterns = remove_ref.patterns(self.lists, np.random.default_rng(3))
        assert list(self.patterns) == remove_ref.PATTERN_NAMES
        self._corpus = None
        self._pqv = pqv

    @property
    def corpus(self):
        if self._corpus is None:
            self._corpus = self._pqv.Corpus.upload(self.X)
        return self._corpus


@pytest.fixture(scope="module")
def cases(pqv, oracle):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(pqv, oracle, name)
        return made[name]
    return get


def _check_index(oracle, index, dim, C, lists, bound):
    off, rows = append_ref.offsets_and_rows(lists)
    assert index.to_bytes() == remove_ref.blob(oracle, dim, C, lists)
    assert np.array_equal(index.list_offsets, off)
    assert np.array_equal(index.list_rows, rows)
    assert index.n_rows == len(rows)
    assert index.row_bound == bound


# remove: every pattern on every index, the three input forms ---------------------------------------------------------------
@pytest.mark.parametrize("pattern", remove_ref.PATTERN_NAMES)
@pytest.mark.parametrize("name", CASES)
def test_remove_equals_the_model(cases, oracle, name, pattern):
    import torch
    c = cases(name)
    flags = c.patterns[pattern]
    want = remove_ref.remove(c.lists, flags)
    got = c.index.remove(flags=flags)                                      # host bytes
    _check_index(oracle, got, c.dim, c.C, want, c.bound)
    blob = got.to_bytes()
    d_flags = torch.from_numpy(flags.copy()).to(torch.device("cuda", 0))
    assert c.index.remove(flags=d_flags).to_bytes() == blob                # device bytes, read in place
    assert c.index.remove(flags=(d_flags.data_ptr(), d_flags.numel())).to_bytes() == blob
    messy = remove_ref.messy_rows(flags, c.bound)                          # row list: any order, duplicates, unindexed ids
    by_rows = c.index.remove(messy)
    assert by_rows.to_bytes() == blob and by_rows.row_bound == c.bound
    assert c.index.to_bytes() == c.blob                                    # the old index is what it was


def test_remove_where_mask_removes_what_the_mask_allows(cases, pqv, oracle):
    c = cases("d72_k128")
    s = pqv.Searcher(c.index, c.corpus)
    allow = np.random.default_rng(1).random(c.n) < 0.25
    mask = s.row_mask(allow)
    got = c.index.remove(where=mask)
    _check_index(oracle, got, c.dim, c.C, remove_ref.remove(c.lists, allow), c.bound)


# chains on an index the GPU built -------------------------------------------------------------------------------------------
def test_chain_append_remove_append_remove(pqv, oracle):
    rng = np.random.default_rng(21)
    dim, k, n0, m1, m2 = 64, 16, 4000, 900, 700
    X = rng.random((n0 + m1 + m2, dim), dtype=np.float32)
    corpus = pqv.Corpus.create(len(X), dim)
    corpus.append(X[:n0])
    index = pqv.IndexBuilder(corpus).n_clusters(k).max_iters(5).workers(1).build()
    C = index.centroids
    lists = index.inverted_lists()

    corpus.append(X[n0:n0 + m1])
    a1 = index.append(corpus)
    lists, _ = append_ref.append_lists(lists, X, C, n0, m1)
    f1 = rng.random(n0 + m1) < 0.4
    f1[-30:] = True                                  # the newest rows leave: the bound stays n0 + m1
    r1 = a1.remove(flags=f1)
    lists = remove_ref.remove(lists, f1)
    assert r1.row_bound == n0 + m1 and append_ref.row_bound(lists) < n0 + m1

    corpus.append(X[n0 + m1:])
    with pytest.raises(pqv.PqvError, match="row bound"):          # refused as before the remove: ids are never reused
        r1.append(corpus, n0 + m1 - 10, 10)
    a2 = r1.append(corpus)                           # continues at the carried bound
    assert a2.row_bound == len(X)
    lists, _ = append_ref.append_lists(lists, X, C, n0 + m1, m2)
    gone = rng.choice(len(X), 1500, replace=False).astype(np.uint32)
    r2 = a2.remove(gone)
    lists = remove_ref.remove_rows(lists, gone)
    _check_index(oracle, r2, dim, C, lists, len(X))
    # the intermediate indexes are what they were
    assert a1.n_rows == n0 + m1 and r1.n_rows == n0 + m1 - int(f1.sum())

    Q = rng.random((8, dim), dtype=np.float32)
    rows, dist, nf, nc = pqv.Searcher(r2, corpus).topk(Q, 10, 4)
    orows, odist, onf, onc = oracle.index_from_parts(dim, C, lists).topk_batch(X, Q, 10, 4)
    assert (nf == onf).all() and (nc == onc).all() and (rows == orows).all() and (_bits(dist) == _bits(odist)).all()
    with pytest.raises(pqv.PqvError, match="out of range for this corpus"):
        pqv.Searcher(r2, pqv.Corpus.upload(X[:n0]))               # ids beyond a smaller corpus are still found


# both list paths: the switch is read once per process, so the host path runs in a child ------------------------------------
_CHILD = """
import hashlib, sys
import numpy as np
sys.path.insert(0, {root!r})
import pq_vector_amd as pqv
X = np.load({x!r})
flags = np.load({f!r})
index = pqv.Index.from_bytes(open({blob!r}, "rb").read())
import torch
d = torch.from_numpy(flags).to(torch.device("cuda", 0))
for new in (index.remove(flags=flags), index.remove(flags=d), index.remove(np.nonzero(flags)[0][::-1])):
    print("REMOVED", hashlib.sha256(new.to_bytes()).hexdigest())
dense, cidx, old_row = new.compact(pqv.Corpus.upload(X))
print("COMPACT", hashlib.sha256(cidx.to_bytes()).hexdigest(), hashlib.sha256(old_row.tobytes()).hexdigest(),
      hashlib.sha256(dense.fetch_rows(np.arange(dense.rows)).tobytes()).hexdigest())
"""


def test_host_list_path_gives_the_same_blobs(cases, oracle, tmp_path):
    c = cases("d72_k128")
    flags = c.patterns["random_0.1"]
    np.save(tmp_path / "x.npy", c.X)
    np.save(tmp_path / "f.npy", flags)
    (tmp_path / "old.blob").write_bytes(c.blob)
    src = _CHILD.format(root=ROOT, x=str(tmp_path / "x.npy"), f=str(tmp_path / "f.npy"), blob=str(tmp_path / "old.blob"))
    out = subprocess.run([sys.executable, "-c", src], env=dict(os.environ, PQV_DEVICE_LISTS="0"), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    removed = remove_ref.remove(c.lists, flags)
    want = hashlib.sha256(remove_ref.blob(oracle, c.dim, c.C, removed)).hexdigest()
    assert out.stdout.count(f"REMOVED {want}") == 3, out.stdout
    X_new, lists_new, old_row = remove_ref.compact(removed, c.X)
    want = " ".join(hashlib.sha256(b).hexdigest() for b in (remove_ref.blob(oracle, c.dim, c.C, lists_new), old_row.astype(np.uint32).tobytes(),
                                                            np.ascontiguousarray(X_new).tobytes()))
    assert f"COMPACT {want}" in out.stdout, out.stdout


# search after remove ----------------------------------------------------------------------------------------------------------
class SearchCase:
    """An index the GPU built, half of its rows removed: the searcher of the removed index against the oracle over the model's
    lists and against the masked call on the old searcher."""

    def __init__(self, pqv, oracle, dim, k, n, seed):
        rng = np.random.default_rng(seed)
        self.dim, self.k, self.n = dim, k, n
        self.X = rng.random((n, dim), dtype=np.float32)
        self.Q = rng.random((32, dim), dtype=np.float32)
        self.corpus = pqv.Corpus.upload(self.X)
        self.index = pqv.IndexBuilder(self.corpus).n_clusters(k).max_iters(5).workers(1).build()
        self.C = self.index.centroids
        self.flags = rng.random(n) < 0.5
        self.old_searcher = pqv.Searcher(self.index, self.corpus)
        self.before = self.old_searcher.topk(self.Q, 10, 4)
        self.removed = self.index.remove(flags=self.flags)
        self.lists = remove_ref.remove(self.index.inverted_lists(), self.flags)
        self.oracle_index = oracle.index_from_parts(dim, self.C, self.lists)


@pytest.fixture(scope="module")
def search_cases(pqv, oracle):
    made = {}

    def get(name):
        if name not in made:
            dim, k, n = {"screened": (64, 16, 8192), "exact": (72, 128, 5000)}[name]
            made[name] = SearchCase(pqv, oracle, dim, k, n, dim)
        return made[name]
    return get


@pytest.mark.parametrize("name", ["screened", "exact"])
def test_search_after_remove(search_cases, pqv, oracle, name):
    c = search_cases(name)
    assert c.removed.to_bytes() == c.oracle_index.to_bytes()
    s = pqv.Searcher(c.removed, c.corpus)
    plan = s.describe(32, 10, 4)
    if name == "screened":          # mean list 256 rows after the remove: above the 192-row rule, the screened kernels serve it
        assert "wide_filter_kernel" in plan, plan
    else:
        assert "wide_filter_kernel" not in plan and "tile_filter_kernel" not in plan, plan
    rows, dist, nf, nc = s.topk(c.Q, 10, 4)
    orows, odist, onf, onc = c.oracle_index.topk_batch(c.X, c.Q, 10, 4)
    assert (nf == onf).all() and (nc == onc).all()
    assert (rows == orows).all()
    assert (_bits(dist) == _bits(odist)).all()
    # ... which is the masked call on the old searcher, n_candidates excepted
    mask = c.old_searcher.row_mask(~c.flags)
    mrows, mdist, mnf, _ = c.old_searcher.topk(c.Q, 10, 4, mask=mask)
    assert (mnf == nf).all() and (mrows == rows).all() and (_bits(mdist) == _bits(dist)).all()
    # ... and the searcher made before the remove answers as before
    after = c.old_searcher.topk(c.Q, 10, 4)
    for a, b in zip(after, c.before):
        assert (_bits(a) == _bits(b)).all() if a.dtype == np.float32 else (a == b).all()


# compact ----------------------------------------------------------------------------------------------------------------------
def _compact_inputs(cases, search_cases, name):
    """-> (index to compact, its model lists, corpus, X, C, dim)"""
    if name == "screened":
        c = search_cases(name)
        return c.removed, c.lists, c.corpus, c.X, c.C, c.dim
    c = cases(name)
    flags = c.patterns["random_0.1"] if name == "hand_made" else (np.arange(c.bound) % 3 == 1)
    return c.index.remove(flags=flags), remove_ref.remove(c.lists, flags), c.corpus, c.X, c.C, c.dim


@pytest.mark.parametrize("name", ["d30_k7", "screened", "d72_k128", "hand_made"])          # dim 30 (scalar gather), 64, 72, 64
def test_compact_equals_the_model(cases, search_cases, pqv, oracle, name):
    removed, lists, corpus, X, C, dim = _compact_inputs(cases, search_cases, name)
    X_new, lists_new, old_row = remove_ref.compact(lists, X)
    kept, extra = len(old_row), 300
    before = removed.to_bytes()
    dense, cidx, got_old = removed.compact(corpus, capacity=kept + extra)
    assert got_old.dtype == np.uint32 and np.array_equal(got_old, old_row)
    assert dense.rows == kept and dense.dim == dim
    assert (_bits(dense.fetch_rows(np.arange(kept))) == _bits(X[old_row])).all()
    _check_index(oracle, cidx, dim, C, lists_new, kept)
    assert cidx.n_rows == kept
    assert removed.to_bytes() == before and corpus.rows == len(X)

    # the searcher goes through the unchecked permutation path (a wrong permutation_of is refused there) ...
    s_new, s_old = pqv.Searcher(cidx, dense), pqv.Searcher(removed, corpus)
    Q = np.random.default_rng(9).random((16, dim), dtype=np.float32)
    rows, dist, nf, nc = s_new.topk(Q, 10, 4)
    rows0, dist0, nf0, nc0 = s_old.topk(Q, 10, 4)
    # ... and answers what the removed index answers, with old_row applied to the ids
    found = rows != 0xFFFFFFFF
    back = np.where(found, old_row[np.where(found, rows, 0)], 0xFFFFFFFF).astype(np.uint32)
    assert (nf == nf0).all() and (nc == nc0).all() and (back == rows0).all() and (_bits(dist) == _bits(dist0)).all()

    # capacity above the kept rows: the ingest step follows on the dense pair
    more = np.random.default_rng(10).random((extra, dim), dtype=np.float32)
    dense.append(more)
    grown = cidx.append(dense)
    X_all = np.concatenate([X_new, more])
    lists_grown, _ = append_ref.append_lists(lists_new, X_all, C, kept, extra)
    _check_index(oracle, grown, dim, C, lists_grown, kept + extra)


def test_compact_default_capacity_and_an_untouched_built_index(pqv):
    rng = np.random.default_rng(31)
    X = rng.random((3000, 30), dtype=np.float32)
    corpus = pqv.Corpus.upload(X)
    index = pqv.IndexBuilder(corpus).n_clusters(7).max_iters(5).workers(1).build()
    dense, cidx, old_row = index.compact(corpus)
    assert cidx.to_bytes() == index.to_bytes()
    assert np.array_equal(old_row, np.arange(3000, dtype=np.uint32))
    assert dense.rows == 3000 and (_bits(dense.fetch_rows(np.arange(3000))) == _bits(X)).all()
    assert cidx.row_bound == 3000
    pqv.Searcher(cidx, dense)
    with pytest.raises(pqv.PqvError, match="capacity"):
        dense.append(X[:1])                          # capacity None: exactly the kept rows


def test_compact_refusals(cases, pqv):
    from pq_vector_amd import _ffi
    c = cases("d30_k7")

    def refused(fn, needle):
        with pytest.raises(pqv.PqvError) as e:
            fn()
        assert e.value.code == _ffi.PQV_ERR_INVALID and needle in e.value.message, e.value.message

    twice = [l.copy() for l in c.lists]
    twice[1] = np.concatenate([twice[1], twice[0][:1]])                    # an index from parts may repeat a row
    refused(lambda: pqv.Index.from_parts(c.dim, c.C, twice).compact(c.corpus), "more than once")
    past = [l.copy() for l in c.lists]
    past[2] = np.concatenate([past[2], np.array([c.n], np.uint32)])        # one id past the corpus
    refused(lambda: pqv.Index.from_parts(c.dim, c.C, past).compact(c.corpus), "index row id out of range for this corpus")
    other = pqv.Corpus.upload(np.zeros((8, c.dim + 2), np.float32))
    refused(lambda: c.index.compact(other), f"index dimension {c.dim} does not match corpus dimension {c.dim + 2}")
    gone = pqv.Corpus.upload(c.X)
    searcher = pqv.Searcher(c.index, gone, flags=_ffi.PQV_RELEASE_ROW_ORDER)
    refused(lambda: c.index.compact(gone), "corpus row-order copy was released")
    del searcher
