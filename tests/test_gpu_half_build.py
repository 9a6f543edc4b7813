"""Index build, assign and append straight from f16 rows (pqv_index_build_f16 / _assign_f16 / _append_f16) against the references
on the rows widened to f32 -- oracle.build_index, assign_exact.nearest, append_ref: index bytes, assignments, row ids and distance
BITS equal, no tolerance (widening is exact).  Shapes: a row shorter than one 128-byte K stage, a partial stage, several stages +
a tail with a part-filled second centroid tile, the exact tier's dword and ushort loads; 3000 rows = 11 row tiles and one of 184."""
import numpy as np
import pytest

import append_ref
import assign_exact

pytestmark = pytest.mark.gpu

N = 3000
EDGE = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x7BFF, 0xFBFF], dtype=np.uint16).view(np.float16)   # +-0, subnormals, +-65504


def _halves(kind, n, dim, seed=0):
    rng = np.random.default_rng(4000 + dim + seed)
    if kind in ("ties", "inf"):          # small integers: many equal distances; "inf": one row steps the whole call down
        h = rng.integers(0, 3, size=(n, dim)).astype(np.float16)
        if kind == "inf":
            h[n // 2, dim // 3] = np.inf
        return h
    if kind == "far":                    # far from the origin: |x| >> |x - mu|, the candidate lists overflow
        return (100.0 + rng.standard_normal((n, dim))).astype(np.float16)
    h = rng.standard_normal((n, dim)).astype(np.float16)
    if kind == "edge":
        flat = h.reshape(-1)
        flat[rng.choice(flat.size, size=64 * len(EDGE), replace=False)] = np.resize(EDGE, 64 * len(EDGE))
    return h


@pytest.mark.parametrize("dim,k,n", [(8, 130, N), (72, 130, N), (264, 300, N), (768, 130, N), (30, 130, N), (7, 12, N), (30, 12, 12)])
def test_build_parity(pqv, oracle, monkeypatch, dim, k, n):
    """the whole build; (30, 12, 12): the training sample is the column (identity gather).  dim % 8 == 0: both tiers"""
    h = _halves("normal", n, dim)
    want = oracle.build_index(h.astype(np.float32), n_clusters=k, workers=4).to_bytes()
    corpus = pqv.Corpus.upload(h)
    assert pqv.IndexBuilder(corpus).n_clusters(k).workers(4).build_f16().to_bytes() == want
    if dim % 8 == 0:
        monkeypatch.setenv("PQV_ASSIGN_GEMM", "0")
        assert pqv.IndexBuilder(corpus).n_clusters(k).workers(4).build_f16().to_bytes() == want


@pytest.mark.parametrize("kind", ["ties", "far", "edge", "inf"])
@pytest.mark.parametrize("dim", [72, 264])
def test_assign_where_the_screen_can_go_wrong(pqv, dim, kind):
    import torch
    k = 300
    h = _halves(kind, N, dim)
    wide = h.astype(np.float32)
    C = _halves("ties" if kind == "inf" else kind, k, dim, seed=1).astype(np.float32)
    want = assign_exact.nearest(wide, C)[0]
    index = pqv.Index.from_parts(dim, C, [np.zeros(0, np.uint32)] * k)
    assert (index.assign_f16(pqv.Corpus.upload(h)) == want).all()
    t = torch.from_numpy(h).cuda()          # a borrowed buffer of exactly n x dim halves: nothing may be read behind it
    borrowed = pqv.Corpus.from_device(t)
    assert (index.assign_f16(borrowed) == want).all()
    assert (index.assign_f16(borrowed, 257, 1000) == want[257:1257]).all()


@pytest.mark.parametrize("value", [0.0, 3.0])
def test_identical_centroids_leave_every_row_in_cluster_0(pqv, value):
    """130 copies of one centroid: every one lies at their mean, the centroid images' scale is degenerate and the screen does not
    decide -- the exact kernel does.  300 rows: one full 256-row tile and a part-filled one; value 3: the mean is not the origin."""
    dim, k, n = 8, 130, 300
    h = _halves("normal", n, dim)
    C = np.full((k, dim), value, np.float32)
    want = assign_exact.nearest(h.astype(np.float32), C)[0]
    assert (want == 0).all()                  # the reference's strict `<`
    index = pqv.Index.from_parts(dim, C, [np.zeros(0, np.uint32)] * k)
    assert (index.assign_f16(pqv.Corpus.upload(h)) == want).all()


def test_append_and_search(pqv, oracle):
    dim, k, n0 = 72, 130, 2000
    h = _halves("normal", N, dim)
    wide = h.astype(np.float32)
    corpus = pqv.Corpus.create(N, dim, dtype=np.float16)
    corpus.append(h[:n0])
    index = pqv.IndexBuilder(corpus).n_clusters(k).workers(4).build_f16()
    old = oracle.build_index(wide[:n0], n_clusters=k, workers=4)
    assert index.to_bytes() == old.to_bytes()
    corpus.append(h[n0:])
    index = index.append_f16(corpus)
    lists = append_ref.append_lists(old.lists(), wide, old.centroids, n0, N - n0)[0]
    assert index.to_bytes() == append_ref.blob(oracle, dim, old.centroids, lists)
    q = np.random.default_rng(9).standard_normal((33, dim)).astype(np.float32)
    got = pqv.Searcher(index, corpus).topk(q, 10, 5)
    exp = oracle.index_from_parts(dim, old.centroids, lists).topk_batch(wide, q, 10, 5)
    for g, e, what in zip(got, exp, ("rows", "dist", "n_found", "n_candidates")):
        g, e = (np.ascontiguousarray(a, np.float32).view(np.uint32) for a in (g, e)) if what == "dist" else (g, e)
        assert (g == e).all(), what


def test_f16_calls_need_f16_rows(pqv):
    corpus = pqv.Corpus.upload(np.zeros((16, 8), np.float32))
    index = pqv.Index.from_parts(8, np.zeros((2, 8), np.float32), [np.zeros(0, np.uint32)] * 2)
    for call in (lambda: pqv.IndexBuilder(corpus).n_clusters(2).build_f16(), lambda: index.assign_f16(corpus), lambda: index.append_f16(corpus, 0, 1)):
        with pytest.raises(pqv.PqvError, match="corpus rows are f32") as e:
            call()
        assert e.value.code == pqv._ffi.PQV_ERR_INVALID
