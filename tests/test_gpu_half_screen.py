"""The screened route of f16 searchers (pqv.h: half-precision corpora, rerank_mode 2: screen_h_kernel + survivor_h_kernel) against the
CPU oracle on the widened rows and a second f16 searcher on the default route (stream_h_kernel): row ids, distance BITS, n_found and
n_candidates equal, no tolerance.  Index as in test_gpu_half.py: lists re-dealt into one row, empty, multi-block."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REF4, SEQ = 0, 1
N, KC, KMAX = 3000, 12, 127       # KMAX: the route's k limit where the list carries the runner-up (pqv.h)
_CASE = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _case(pqv, oracle, dim, hostile=0):
    """(widened rows, oracle index, screened f16 searcher, default f16 searcher, 70 queries), built once per shape"""
    if (dim, hostile) not in _CASE:
        rng = np.random.default_rng(1000 + dim + (7 if hostile else 0))
        if hostile:       # small integers: many equal distances; 2: a few rows with Inf / NaN halves
            h = rng.integers(0, 3, size=(N, dim)).astype(np.float16)
            if hostile == 2:
                h[rng.choice(N, size=6, replace=False), 0] = np.array([np.inf, -np.inf, np.nan, np.inf, np.nan, -np.inf], dtype=np.float16)
        else:
            h = rng.standard_normal((N, dim)).astype(np.float16)
            edge = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x7BFF, 0xFBFF], dtype=np.uint16).view(np.float16)   # +-0, subnormals, +-65504
            flat = h.reshape(-1)
            flat[rng.choice(flat.size, size=8 * len(edge), replace=False)] = np.resize(edge, 8 * len(edge))
        wide = h.astype(np.float32)
        cents = oracle.build_index(np.clip(np.nan_to_num(wide, posinf=4, neginf=-4), -4, 4), n_clusters=KC, workers=4).centroids
        order = np.argsort(rng.integers(0, KC, size=N), kind="stable").astype(np.uint32)
        cuts = [0, 1, 1, 1301] + list(np.linspace(1301, N, KC - 2).astype(int)[1:])       # list 0 one row, list 1 empty, list 2 > 1024 rows
        lists = [order[cuts[i]:cuts[i + 1]] for i in range(KC)]
        index = pqv.Index.from_parts(dim, cents, lists)
        s2 = pqv.Searcher(index, pqv.Corpus.upload(h)).set_option("rerank_mode", 2)
        queries = np.random.default_rng(5007 + dim).standard_normal((70, dim)).astype(np.float32)
        _CASE[(dim, hostile)] = (wide, oracle.index_from_parts(dim, cents, lists), s2, pqv.Searcher(index, pqv.Corpus.upload(h)), queries)
    return _CASE[(dim, hostile)]


def _same(got, exp, upto_found=False):
    """upto_found: behind n_found the library pads with 0xFFFFFFFF / inf, the oracle binding with zeros"""
    assert (got[2] == exp[2]).all() and (got[3] == exp[3]).all(), "n_found / n_candidates"
    for i, nf in enumerate(got[2]):
        n = nf if upto_found else got[0].shape[1]
        assert (got[0][i, :n] == exp[0][i, :n]).all() and (_bits(got[1][i, :n]) == _bits(exp[1][i, :n])).all(), ("rows / distance bits", i)


def _device(s, queries, k, nprobe, flags, **kw):
    import torch
    q = torch.from_numpy(queries).cuda()
    nq = len(queries)
    rows = torch.zeros((nq, k), dtype=torch.int32, device="cuda")
    dist = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
    nf = torch.zeros(nq, dtype=torch.int32, device="cuda")
    nc = torch.zeros(nq, dtype=torch.int64, device="cuda")
    tie = torch.zeros(nq, dtype=torch.int32, device="cuda")
    s.topk_device(q.data_ptr(), nq, k, nprobe, rows.data_ptr(), dist.data_ptr(), nf.data_ptr(), nc.data_ptr(),
                  d_tie_flags=tie.data_ptr() if flags else 0, **kw)
    torch.cuda.synchronize()
    return (rows.cpu().numpy().view(np.uint32), dist.cpu().numpy(), nf.cpu().numpy().view(np.uint32), nc.cpu().numpy().view(np.uint64)), tie.cpu().numpy()


def _ran(s2, c0, nq, k, nprobe, half):
    """the route ran: named by describe, pairs screened, some but not all of them evaluated exactly (half: at most every second)"""
    c1 = s2.counters()
    pairs, surv = c1["screened_pairs"] - c0["screened_pairs"], c1["screen_survivors"] - c0["screen_survivors"]
    print(f"screened_pairs {pairs} screen_survivors {surv}")
    assert "screen_h_kernel" in s2.describe(nq, k, nprobe) and "survivor_h_kernel" in s2.describe(nq, k, nprobe)
    assert pairs > 0 and 0 < surv < pairs
    assert not half or 2 * surv <= pairs


@pytest.mark.parametrize("dim", [8, 24, 72, 256, 264, 768])
def test_screen_dims(pqv, oracle, dim):
    """less than one K stage, a partial stage, an odd count of 32-value chunks, the headline width; 70 queries: two tiles on a list"""
    wide, oidx, s2, sh, queries = _case(pqv, oracle, dim)
    for nq in (1, 33, 70):
        q, c0 = queries[:nq], s2.counters()
        got = s2.topk(q, 10, 5)
        _ran(s2, c0, nq, 10, 5, True)
        _same(got, oidx.topk_batch(wide, q, 10, 5), upto_found=True)
        _same(got, sh.topk(q, 10, 5))


@pytest.mark.parametrize("k,nprobe,cap,sqrt_out", [(1, 5, 0, False), (10, 5, 0, False), (100, 5, 0, False), (KMAX, 5, 0, False), (10, 1, 0, False),
                                                   (10, 64, 0, False), (10, 5, 1500, False), (10, 5, 0, True), (100, 64, 1500, False)])       # (d2 out at k 100: sqrt rounds neighbouring distances together)
@pytest.mark.parametrize("dim", [24, 264])
def test_screen_parameters(pqv, oracle, dim, k, nprobe, cap, sqrt_out):
    """each axis against the base case, host form and both device forms"""
    wide, oidx, s2, sh, queries = _case(pqv, oracle, dim)
    q, kw = queries[:33], dict(max_candidates=cap, sqrt_out=sqrt_out)
    c0 = s2.counters()
    exp = sh.topk(q, k, nprobe, **kw)
    _same(s2.topk(q, k, nprobe, **kw), exp)
    _ran(s2, c0, 33, k, nprobe, k == 10 and nprobe == 5)
    if not cap:
        _same(s2.topk(q, k, nprobe), oidx.topk_batch(wide, q, k, nprobe), upto_found=True)
    got, tie = _device(s2, q, k, nprobe, True, **kw)
    assert (tie == 0).all(), "continuous data must not tie (a condition on the inputs)"
    _same(got, exp)
    _same(_device(s2, q, k, nprobe, False, **kw)[0], exp)


def test_screen_hostile(pqv, oracle):
    """equal distances everywhere: the host form equals the oracle, the device flags the default route's; then with Inf / NaN rows and
    non-finite queries on top: the default route's results, bits included"""
    for hostile in (1, 2):
        wide, oidx, s2, sh, queries = _case(pqv, oracle, 24, hostile)
        q = np.round(queries[:33]).astype(np.float32)
        if hostile == 1:
            _same(s2.topk(q, 10, 5), oidx.topk_batch(wide, q, 10, 5), upto_found=True)
        else:
            q[5, 3], q[9, 0] = np.inf, np.nan
            _same(s2.topk(q, 10, 5), sh.topk(q, 10, 5))
        got, tie = _device(s2, q, 10, 5, True)
        ref, rtie = _device(sh, q, 10, 5, True)
        assert tie.any() and (tie == rtie).all()
        keep = tie == 0
        assert (got[0][keep] == ref[0][keep]).all() and (_bits(got[1][keep]) == _bits(ref[1][keep])).all() and (got[2] == ref[2]).all()


@pytest.mark.parametrize("dim,k,metric", [(30, 10, REF4), (24, 10, SEQ), (24, KMAX + 1, REF4)])
def test_screen_fall_through(pqv, oracle, dim, k, metric):
    """where the route does not apply rerank_mode 2 changes nothing: the default route's results, and describe says so"""
    wide, oidx, s2, sh, queries = _case(pqv, oracle, dim)
    c0 = s2.counters()
    _same(s2.topk(queries[:33], k, 5, metric=metric, sqrt_out=False), sh.topk(queries[:33], k, 5, metric=metric, sqrt_out=False))
    assert "stream_h_kernel" in s2.describe(33, k, 5, metric) and s2.counters()["screened_pairs"] == c0["screened_pairs"]
