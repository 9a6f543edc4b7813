"""Index append on the GPU (pqv_index_assign / pqv_index_append, IndexBuilder.with_centroids): every expectation comes from code that
is not under test -- the assignment from tests/assign_exact.py, the lists from the numpy model tests/append_ref.py (old list ++
first_row + ascending new rows), the blobs from the oracle's index_from_parts.  Shapes are the smallest that reach each form of
the assignment stage (exact kernel: dim 30; f16 contraction: dim 72 x 128 centroids and dim 64 x 512 centroids) and each list
path (device sort + splice kernel up to 4096 clusters, host splice above)."""
import numpy as np
import pytest

import append_ref
import assign_exact

pytestmark = pytest.mark.gpu

M_MAX = 1300
# name -> (dim, k, n0): the old index covers rows [0, n0), up to M_MAX rows follow
SHAPES = {"exact_d30_k7": (30, 7, 3000), "gemm_d72_k128": (72, 128, 5000), "gemm_d64_k512": (64, 512, 6000)}
SEEDS = {"exact_d30_k7": 30, "gemm_d72_k128": 72, "gemm_d64_k512": 64}
GEMM_M = (1, 255, 257, 1300)      # one row; one short of / one past a 256-row tile or list-sort block; several blocks


class Case:
    def __init__(self, pqv, oracle, name):
        self.dim, self.k, self.n0 = SHAPES[name]
        rng = np.random.default_rng(SEEDS[name])
        self.X = rng.random((self.n0 + M_MAX, self.dim), dtype=np.float32)
        oidx = oracle.build_index(self.X[:self.n0], n_clusters=self.k, max_iters=5, workers=1)
        self.old_blob = oidx.to_bytes()
        self.C = oidx.centroids
        self.old_lists = oidx.lists()
        self.assign = assign_exact.nearest(self.X[self.n0:], self.C)[0]          # rows n0 .. n0 + M_MAX, once
        self.corpus = pqv.Corpus.upload(self.X)
        self.index = pqv.Index.from_bytes(self.old_blob)

    def lists(self, m, first=None):
        first = self.n0 if first is None else first
        return append_ref.splice(self.old_lists, self.assign[first - self.n0:first - self.n0 + m], first)


@pytest.fixture(scope="module")
def cases(pqv, oracle):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(pqv, oracle, name)
        return made[name]
    return get


def _shape_m():
    out = [("exact_d30_k7", 1000)]
    for name in ("gemm_d72_k128", "gemm_d64_k512"):
        out += [(name, m) for m in GEMM_M]
    return out


def _check_index(oracle, index, dim, C, lists):
    off, rows = append_ref.offsets_and_rows(lists)
    assert index.to_bytes() == append_ref.blob(oracle, dim, C, lists)
    assert np.array_equal(index.list_offsets, off)
    assert np.array_equal(index.list_rows, rows)
    assert index.n_rows == len(rows)


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,m", _shape_m())
def test_assign_of_a_sub_range(cases, name, m):
    c = cases(name)
    got = c.index.assign(c.corpus, c.n0, m)
    assert got.dtype == np.uint32 and got.shape == (m,)
    assert assign_exact.mismatches(c.X[c.n0:c.n0 + m], c.C, got, c.assign[:m]) is None


def test_assign_defaults_cover_the_whole_corpus(cases):
    c = cases("exact_d30_k7")
    got = c.index.assign(c.corpus)
    want = np.concatenate([assign_exact.nearest(c.X[:c.n0], c.C)[0], c.assign])
    assert assign_exact.mismatches(c.X, c.C, got, want) is None


# 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,m", _shape_m())
def test_append_blob(cases, oracle, name, m):
    c = cases(name)
    new = c.index.append(c.corpus, c.n0, m)
    _check_index(oracle, new, c.dim, c.C, c.lists(m))
    assert new.row_bound == c.n0 + m
    assert c.index.to_bytes() == c.old_blob


def test_append_defaults_and_the_reference_blob(cases):
    """first_row defaults to the row bound (found by the host scan of a from_bytes index), n_rows to the end of the corpus; the old
    lists are the nearest lists of rows [0, n0), so the result is the reference's blob for these centroids over all rows."""
    import build_reference
    c = cases("gemm_d72_k128")
    assert c.index.row_bound == c.n0
    new = c.index.append(c.corpus)
    full = np.concatenate([assign_exact.nearest(c.X[:c.n0], c.C)[0], c.assign])
    assert new.to_bytes() == build_reference.reference_blob(c.dim, c.C, full, c.k)[0]


# 3, 4 ---------------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("dim,k,n0,m", [(30, 16, 3000, 700), (64, 16, 4000, 900)])
def test_append_to_an_index_the_gpu_built_and_old_searcher_undisturbed(pqv, oracle, dim, k, n0, m):
    rng = np.random.default_rng(dim)
    X = rng.random((n0 + m, dim), dtype=np.float32)
    Q = rng.random((8, dim), dtype=np.float32)
    corpus = pqv.Corpus.create(n0 + m, dim)
    corpus.append(X[:n0])
    index = pqv.IndexBuilder(corpus).n_clusters(k).max_iters(5).workers(1).build()
    old_searcher = pqv.Searcher(index, corpus)
    before = old_searcher.topk(Q, 10, 4)

    corpus.append(X[n0:])
    new = index.append(corpus)               # the old lists come from the build's device copy; permutation_of carries over
    C = index.centroids
    old_lists = index.inverted_lists()
    assert sum(len(l) for l in old_lists) == n0
    lists, _ = append_ref.append_lists(old_lists, X, C, n0, m)
    _check_index(oracle, new, dim, C, lists)

    rows, dist, nf, nc = pqv.Searcher(new, corpus).topk(Q, 10, 4)
    orows, odist, onf, onc = oracle.index_from_bytes(new.to_bytes()).topk_batch(X, Q, 10, 4)
    assert (nf == onf).all() and (nc == onc).all()
    assert (rows == orows).all()
    assert (_bits(dist) == _bits(odist)).all()

    after = old_searcher.topk(Q, 10, 4)      # 4: the searcher made before the corpus grew
    assert (after[0] == before[0]).all() and (_bits(after[1]) == _bits(before[1])).all()
    assert (after[2] == before[2]).all() and (after[3] == before[3]).all()
    # ... and a new searcher from the OLD index on the grown corpus keeps failing as before
    with pytest.raises(pqv.PqvError, match="out of range for this corpus"):
        pqv.Searcher(index, corpus)
    assert new.append(corpus, n0 + m, 0).to_bytes() == new.to_bytes()


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_chain_split_empty_and_gap(cases, pqv, oracle):
    c = cases("gemm_d72_k128")
    n0, n1, n2 = c.n0, c.n0 + 300, c.n0 + 1300
    once = c.index.append(c.corpus, n0, n2 - n0)
    step = c.index.append(c.corpus, n0, n1 - n0)
    assert step.row_bound == n1
    twice = step.append(c.corpus)            # [n1, n2): the device copy of `step` is the old list source
    assert twice.to_bytes() == once.to_bytes()
    _check_index(oracle, twice, c.dim, c.C, c.lists(n2 - n0))

    assert c.index.append(c.corpus, n0, 0).to_bytes() == c.old_blob
    assert once.append(c.corpus, n2, 0).to_bytes() == once.to_bytes()

    first = c.index.row_bound + 17
    gap = c.index.append(c.corpus, first, n2 - first)
    lists = c.lists(n2 - first, first)
    _check_index(oracle, gap, c.dim, c.C, lists)
    indexed = np.sort(np.concatenate(lists))
    assert np.array_equal(indexed, np.concatenate([np.arange(n0), np.arange(first, n2)]))
    Q = c.X[[3, n0 + 5, n0 + 40, n2 - 1]]
    rows, dist, nf, nc = pqv.Searcher(gap, c.corpus).topk(Q, 10, 4)
    orows, odist, onf, onc = oracle.index_from_bytes(gap.to_bytes()).topk_batch(c.X, Q, 10, 4)
    assert (nf == onf).all() and (rows == orows).all() and (_bits(dist) == _bits(odist)).all()


# 6 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["exact_d30_k7", "gemm_d72_k128"])
def test_old_lists_are_kept_not_recomputed(cases, pqv, oracle, name):
    c = cases(name)
    wrong = [np.arange(j, c.n0, c.k, dtype=np.uint32) for j in range(c.k)]          # rows dealt round robin
    old = pqv.Index.from_parts(c.dim, c.C, wrong)
    new = old.append(c.corpus)
    got = new.inverted_lists()
    for j in range(c.k):
        assert np.array_equal(got[j][:len(wrong[j])], wrong[j])
    _check_index(oracle, new, c.dim, c.C, append_ref.splice(wrong, c.assign, c.n0))


# 7 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,k", [(30, 7), (72, 128)])
def test_ties_go_to_the_lower_index(pqv, oracle, dim, k):
    rng = np.random.default_rng(k)
    n0, m = 500, 600
    X = rng.integers(0, 3, (n0 + m, dim)).astype(np.float32)
    C = rng.integers(0, 3, (k, dim)).astype(np.float32)
    C[1] = X[n0:].mean(axis=0).round()        # a centroid in the middle of the data takes many rows ...
    C[k - 2] = C[1]                           # ... and its copy at a higher index must take none
    want = assign_exact.nearest(X[n0:], C)[0]
    assert (want == 1).sum() > 0 and (want == k - 2).sum() == 0
    index = pqv.Index.from_parts(dim, C, [np.zeros(0, np.uint32)] * k)
    corpus = pqv.Corpus.upload(X)
    got = index.assign(corpus, n0, m)
    assert assign_exact.mismatches(X[n0:], C, got, want) is None
    _check_index(oracle, index.append(corpus, n0, m), dim, C, append_ref.splice([[]] * k, want, n0))


@pytest.mark.parametrize("name", ["exact_d30_k7", "gemm_d72_k128"])
def test_non_finite_rows(cases, pqv, oracle, name):
    c = cases(name)
    m = 600
    X = c.X[:c.n0 + m].copy()
    X[c.n0 + 100, 3] = np.nan
    X[c.n0 + 300, 5] = np.inf
    with np.errstate(all="ignore"):
        want = assign_exact.nearest(X[c.n0:], c.C)[0]
    corpus = pqv.Corpus.upload(X)
    got = c.index.assign(corpus, c.n0, m)
    assert assign_exact.mismatches(X[c.n0:], c.C, got, want) is None
    _check_index(oracle, c.index.append(corpus, c.n0, m), c.dim, c.C, append_ref.splice(c.old_lists, want, c.n0))

    # a NaN in an OLD row: outside the range, it changes nothing
    X = c.X[:c.n0 + m].copy()
    X[7, 1] = np.nan
    corpus = pqv.Corpus.upload(X)
    got = c.index.assign(corpus, c.n0, m)
    assert assign_exact.mismatches(X[c.n0:], c.C, got, c.assign[:m]) is None
    _check_index(oracle, c.index.append(corpus, c.n0, m), c.dim, c.C, c.lists(m))


# 8 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [4096, 4100])
def test_list_paths_on_both_sides_of_the_device_limit(pqv, oracle, k):
    """4096 clusters: the largest table the device sort and the splice kernel take (both offset tables in LDS); 4100: the host
    splice.  Few rows per list and many empty lists; the second append extends non-empty old lists."""
    rng = np.random.default_rng(8)
    dim, n1, n2 = 4, 5000, 8000
    C = rng.random((k, dim), dtype=np.float32)
    X = rng.random((n2, dim), dtype=np.float32)
    index = pqv.Index.from_parts(dim, C, [np.zeros(0, np.uint32)] * k)
    assert index.row_bound == 0
    corpus = pqv.Corpus.upload(X)
    first = index.append(corpus, 0, n1)
    want = assign_exact.nearest(X, C)[0]
    lists1 = append_ref.splice([[]] * k, want[:n1], 0)
    second = first.append(corpus)
    _check_index(oracle, second, dim, C, append_ref.splice(lists1, want[n1:], n1))
    _check_index(oracle, first, dim, C, lists1)


# 9 ------------------------------------------------------------------------------------------------------------------------
def test_with_centroids(cases, pqv, oracle, tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    c = cases("gemm_d72_k128")
    rng = np.random.default_rng(9)
    B = rng.random((700, c.dim), dtype=np.float32)
    want_lists = append_ref.splice([[]] * c.k, assign_exact.nearest(B, c.C)[0], 0)
    want = append_ref.blob(oracle, c.dim, c.C, want_lists)

    built = pqv.IndexBuilder(B).with_centroids(c.index).max_iters(0).build()       # max_iters is ignored
    assert built.to_bytes() == want
    assert pqv.IndexBuilder(pqv.Corpus.upload(B)).with_centroids(c.C).n_clusters(c.k).build().to_bytes() == want
    rows, dist, nf, nc = pqv.Searcher(built, pqv.Corpus.upload(B)).topk(B[:4], 5, 3)
    orows, odist, onf, onc = oracle.index_from_bytes(want).topk_batch(B, B[:4], 5, 3)
    assert (rows == orows).all() and (_bits(dist) == _bits(odist)).all()

    with pytest.raises(pqv.PqvError) as e:
        pqv.IndexBuilder(B).with_centroids(c.index).n_clusters(c.k + 1).build()
    assert e.value.code == pqv._ffi.PQV_ERR_INVALID and "does not match" in e.value.message
    # more centroids than rows is fine here: that rule is k-means'
    few = pqv.IndexBuilder(B[:50]).with_centroids(c.index).build()
    assert few.n_rows == 50 and few.n_clusters == c.k

    src, out = str(tmp_path / "b.parquet"), str(tmp_path / "b_indexed.parquet")
    col = pa.array(B.tolist(), type=pa.list_(pa.field("item", pa.float32())))
    pq.write_table(pa.table({"id": pa.array(np.arange(len(B), dtype=np.int32)), "vec": col}), src, row_group_size=256)
    made = pqv.IndexBuilder(src, "vec").with_centroids(c.index).build_new(out)
    assert made.to_bytes() == want
    back, name = pqv.read_index_from_parquet(out)
    assert name == "vec" and back.to_bytes() == want
    assert pqv.Index.from_bytes(back.to_bytes()).to_bytes() == want


# 10 -----------------------------------------------------------------------------------------------------------------------
def test_errors_through_a_real_corpus(cases, pqv):
    import ctypes as C
    from pq_vector_amd import _ffi
    c = cases("exact_d30_k7")
    n = c.corpus.rows
    seen = []

    def refused(fn):
        with pytest.raises(pqv.PqvError) as e:
            fn()
        assert e.value.code == _ffi.PQV_ERR_INVALID and e.value.message
        seen.append(e.value.message)
        return e.value.message

    assert "row bound" in refused(lambda: c.index.append(c.corpus, c.n0 - 1, 10))
    assert "out of range" in refused(lambda: c.index.append(c.corpus, c.n0, n - c.n0 + 1))
    assert "out of range" in refused(lambda: c.index.assign(c.corpus, n - 5, 6))
    other = pqv.Corpus.upload(np.zeros((8, c.dim + 2), np.float32))
    msg = refused(lambda: c.index.append(other, c.n0, 0))
    assert msg == f"index dimension {c.dim} does not match corpus dimension {c.dim + 2}"
    refused(lambda: c.index.assign(other, 0, 1))
    assert seen[-1] == msg

    gone = pqv.Corpus.upload(c.X[:c.n0 + 50])
    searcher = pqv.Searcher(c.index.append(gone), gone, flags=_ffi.PQV_RELEASE_ROW_ORDER)
    assert refused(lambda: c.index.append(gone)) == "corpus row-order copy was released"
    assert refused(lambda: c.index.assign(gone, 0, 4)) == "corpus row-order copy was released"
    del searcher
    assert len({seen[0], seen[1], msg, "corpus row-order copy was released"}) == 4

    # NULL cluster_out / out with a real index and corpus
    lib = _ffi.lib()
    assert lib.pqv_index_assign(c.index._h, c.corpus._h, 0, 4, C.cast(None, _ffi.u32p)) == _ffi.PQV_ERR_INVALID
    assert "cluster_out" in lib.pqv_last_error().decode()
    assert lib.pqv_index_append(c.index._h, c.corpus._h, c.n0, 4, C.cast(None, C.POINTER(_ffi.vp))) == _ffi.PQV_ERR_INVALID
    assert "out must not be NULL" in lib.pqv_last_error().decode()


# the list switches of the build apply to an append too: read once per process, so each runs in a child ------------------------
_CHILD = """
import hashlib, sys
import numpy as np
sys.path.insert(0, {root!r})
import pq_vector_amd as pqv
X = np.load({x!r})
index = pqv.Index.from_bytes(open({blob!r}, "rb").read())
new = index.append(pqv.Corpus.upload(X)).append(pqv.Corpus.upload(X), {n1}, 0)
print("BLOB", hashlib.sha256(new.to_bytes()).hexdigest())
"""


@pytest.mark.parametrize("switch", ["PQV_DEVICE_LISTS", "PQV_KEEP_DEVICE_LISTS"])
def test_list_switches_give_the_same_blob(cases, oracle, tmp_path, switch):
    import hashlib
    import os
    import subprocess
    import sys
    c = cases("gemm_d72_k128")
    m = 257
    np.save(tmp_path / "x.npy", c.X[:c.n0 + m])
    (tmp_path / "old.blob").write_bytes(c.old_blob)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = _CHILD.format(root=root, x=str(tmp_path / "x.npy"), blob=str(tmp_path / "old.blob"), n1=c.n0 + m)
    out = subprocess.run([sys.executable, "-c", src], env=dict(os.environ, **{switch: "0"}), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    want = hashlib.sha256(append_ref.blob(oracle, c.dim, c.C, c.lists(m))).hexdigest()
    assert f"BLOB {want}" in out.stdout
