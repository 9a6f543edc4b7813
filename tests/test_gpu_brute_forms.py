"""pqv_brute_topk where its screen actually runs (from 32 768 rows on): every brute_f16_kernel form launch_brute_f16 can select, at
the K-stage counts where its loop changes shape, the host schedule's edges (k, sub-batches, a growing corpus, the roll-back and
split of an overflowing range) -- each answer against the f64 reference and the project's acceptance rule (brute_ref.py).

The sharper check: every screened form re-scores its survivors with the same brute_rescore_kernel, selects by the same key and
takes the first row range through the same f32 kernel.  If every screen is a true bound, all of them -- int8, f16, ring, each tile
and stage width -- return bit-identical rows and distances for the same call.  A difference means one screen dropped a row that
the exact pass ranks inside the top k."""
import os
import subprocess
import sys

import numpy as np
import pytest

import brute_ref as br

pytestmark = pytest.mark.gpu

N, K = br.N_FORMS, 10
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _metric(pqv, metric):
    return pqv.PQV_COSINE if metric == br.COS else pqv.PQV_L2SQ_MFMA


def _call(pqv, monkeypatch, corpus, queries, k, metric, op):
    """op: i8 | f16 | i8-ring | f16-ring (both switches are read per call)"""
    monkeypatch.setenv("PQV_BRUTE_OP", op.split("-")[0])
    monkeypatch.setenv("PQV_BRUTE_RING", "1" if op.endswith("ring") else "0")
    return corpus.brute_topk(queries, k, _metric(pqv, metric))


def _all_ops(pqv, monkeypatch, corpus, ref, k, ops, what):
    """one call per op on ref's queries: each against the reference, all of them bit-identical; returns the answer"""
    got = {}
    for op in ops:
        got[op] = _call(pqv, monkeypatch, corpus, ref.queries, k, ref.metric, op)
        br.check(ref, k, *got[op], what=f"{what}, {op}")
    for op in ops[1:]:
        br.assert_same_bits(got[ops[0]], got[op], f"{what}: {ops[0]} against {op}")
    return got[ops[0]]


# ---------------------------------------------------------------------------------------
# a. forms x stage counts.  Image rows: int8 dim rounded up to 64 bytes, f16 2 x (dim rounded up to 32 values).
#      dim            7    32    50    64    96   100   160   256   1536
#      int8 bytes    64    64    64    64   128   128   192   256   1536
#      f16 bytes     64    64   128   128   192   256   320   512   3072
#    33 queries: the 128 x 256 tile (64-byte stages).  130 queries: the 256 x 256 tile, 128-byte stages where the image row is a
#    multiple of 128 bytes (nk = 1, 2, 4, 12, 24), else 64-byte stages (nk = 1, 3, 5); the ring walks 64-byte stages
#    (nk = 1, 2, 3, 4, 5, 8, 24, 48: every case of its prologue and of its counted waits).
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim", br.FORM_CASES, ids=[f"{k}-{d}" for k, d in br.FORM_CASES])
def test_every_form_matches_the_reference_and_every_other_form(pqv, monkeypatch, kind, dim):
    data, queries = br.make_case(kind, N, dim, 130)
    corpus = pqv.Corpus.upload(data)
    try:
        for metric in (br.COS, br.L2):
            ref = br.reference(data, queries, K, metric)
            _all_ops(pqv, monkeypatch, corpus, ref.take(slice(0, 33)), K, ["i8", "f16"], f"{kind} {dim} {metric} nq 33")
            _all_ops(pqv, monkeypatch, corpus, ref, K, ["i8", "f16", "i8-ring", "f16-ring"], f"{kind} {dim} {metric} nq 130")
    finally:
        corpus.close()


# ---------------------------------------------------------------------------------------
# b. shape edges
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge(pqv):
    data, queries = br.make_case("normal", N, 64, 257)
    corpus = pqv.Corpus.upload(data)
    refs = {}

    def ref(metric):
        if metric not in refs:
            refs[metric] = br.reference(data, queries, 1024, metric)
        return refs[metric]
    yield corpus, ref
    corpus.close()


@pytest.mark.parametrize("metric", [br.COS, br.L2])
def test_query_counts_around_the_tile_sizes(pqv, monkeypatch, edge, metric):
    corpus, ref = edge
    for nq in (1, 128, 129, 256, 257):
        _all_ops(pqv, monkeypatch, corpus, ref(metric).take(slice(0, nq)), K, ["i8", "f16"], f"{metric} nq {nq}")


@pytest.mark.parametrize("metric", [br.COS, br.L2])
def test_k_around_the_select_kernel_sizes(pqv, monkeypatch, edge, metric):
    """brute_select_kernel<1> to k = 64, <4> to 256, <16> to 1024 (where the first, exact range grows to 8 k = 8192 rows)"""
    corpus, ref = edge
    r = ref(metric).take(slice(0, 130))
    for k in (1, 64, 65, 256, 257, 1024):
        _all_ops(pqv, monkeypatch, corpus, r, k, ["i8", "f16"], f"{metric} k {k}")


def test_k_beyond_1024_is_refused(pqv, edge):
    corpus, ref = edge
    with pytest.raises(pqv.PqvError, match="k > 1024 is not supported"):
        corpus.brute_topk(ref(br.COS).queries[:2], 1025)


@pytest.mark.parametrize("metric", [br.COS, br.L2])
def test_second_query_sub_batch(pqv, monkeypatch, metric):
    """4097 queries: a sub-batch of 4096 and one of a single query"""
    data, queries = br.make_case("normal", N, 32, 4097)
    corpus = pqv.Corpus.upload(data)
    try:
        sel = np.r_[0:64, 4090:4097]
        ref = br.reference(data, queries[sel], K, metric)
        got = {}
        for op in ("i8", "f16"):
            got[op] = _call(pqv, monkeypatch, corpus, queries, K, metric, op)
            br.check_order(*got[op], N, K)
            br.check(ref, K, *(a[sel] for a in got[op]), what=f"{metric} {op}")
            alone = _call(pqv, monkeypatch, corpus, queries[4096:], K, metric, op)
            br.assert_same_bits(tuple(a[4096:] for a in got[op]), alone, f"{metric} {op}: query 4096 in the batch against the same query alone")
        br.assert_same_bits(got["i8"], got["f16"], f"{metric}: i8 against f16")
    finally:
        corpus.close()


@pytest.mark.parametrize("metric", [br.COS, br.L2])
def test_row_tile_counts_0_and_1_mod_8(pqv, monkeypatch, metric):
    """n = 32768 + 2048 + 1: the range [2048, 18432) is 64 row tiles (a full round of the 8 XCDs), [18432, n) is 64 tiles and one row"""
    n = 32768 + 256 * 8 + 1
    data, queries = br.make_case("normal", n, 64, 130)
    corpus = pqv.Corpus.upload(data)
    try:
        ref = br.reference(data, queries, K, metric)
        _all_ops(pqv, monkeypatch, corpus, ref.take(slice(0, 33)), K, ["i8", "f16"], f"{metric} nq 33")
        _all_ops(pqv, monkeypatch, corpus, ref, K, ["i8", "f16", "i8-ring", "f16-ring"], f"{metric} nq 130")
    finally:
        corpus.close()


# ---------------------------------------------------------------------------------------
# c. roll-back and split
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [br.COS, br.L2])
def test_overflowing_ranges_are_rolled_back_and_split(pqv, monkeypatch, capfd, metric):
    """Rows sorted towards the queries: every row of a new range beats the thresholds so far, so [2048, 18432) appends
    k + 16384 > cap = 16384 entries per query and must be rolled back and halved (as must [18432, n), and [8192, n) of the f32-only
    schedule below 32 768 rows).  Same answer as the reference, from both screens bit for bit, and no minimal-range error."""
    dim, nq = 64, 130
    for n in (36_000, 30_000):
        data, queries = br.make_sorted_towards_queries(n, dim, nq)
        br.assert_ranges_overflow(data, queries, K, metric, 2048, 18432)     # the pre-condition, from the reference alone
        br.assert_ranges_overflow(data, queries, K, metric, 8192, n)
        if n >= 32768:
            br.assert_ranges_overflow(data, queries, K, metric, 18432, n)
        ref = br.reference(data, queries, K, metric)
        corpus = pqv.Corpus.upload(data)
        try:
            monkeypatch.setenv("PQV_BRUTE_STATS", "1")
            capfd.readouterr()
            _all_ops(pqv, monkeypatch, corpus, ref, K, ["i8", "f16"], f"{metric} n {n}")
            err = capfd.readouterr().err
            monkeypatch.delenv("PQV_BRUTE_STATS")
        finally:
            corpus.close()
        if n >= 32768:          # the diagnostic names the ranges that were screened to the end: the halves, never the whole
            assert err.count("rows [2048, 10240)") == 2 and err.count("rows [10240, 18432)") == 2, err
            assert "rows [2048, 18432)" not in err and f"rows [18432, {n})" not in err, err
        else:
            assert "screen survivors" not in err, err                         # no screen below 32 768 rows


# ---------------------------------------------------------------------------------------
# d. a growing corpus
# ---------------------------------------------------------------------------------------
def test_corpus_growing_past_the_screen_threshold(pqv, monkeypatch):
    """30 000 rows (the f32-only path), then 5 001 more: the norms and both images are rebuilt for the grown corpus, the rows
    planted among the new ones come first, and the answer is the one of a fresh upload of the same rows, bit for bit."""
    dim, nq = 64, 130
    data, queries = br.make_case("normal", N, dim, nq)
    rng = np.random.default_rng(5)
    planted = 30_000 + 600 * np.arange(8) + 17
    data[planted] = queries[:8] + np.float32(1e-3) * rng.standard_normal((8, dim)).astype(np.float32)
    grown = pqv.Corpus.create(40_000, dim)
    fresh = pqv.Corpus.upload(data)
    try:
        grown.append(data[:30_000])
        for metric in (br.COS, br.L2):
            br.check(br.reference(data[:30_000], queries, K, metric), K, *_call(pqv, monkeypatch, grown, queries, K, metric, "i8"),
                     what=f"{metric}, 30 000 rows")
        grown.append(data[30_000:])
        assert grown.rows == N
        for metric in (br.COS, br.L2):
            ref = br.reference(data, queries, K, metric)
            for op in ("i8", "f16"):
                got = _call(pqv, monkeypatch, grown, queries, K, metric, op)
                assert np.array_equal(got[0][:8, 0], planted.astype(np.uint32)), f"{metric} {op}: the planted rows are not first"
                br.check(ref, K, *got, what=f"{metric} {op}, grown")
                br.assert_same_bits(got, _call(pqv, monkeypatch, fresh, queries, K, metric, op), f"{metric} {op}: grown against a fresh upload")
    finally:
        grown.close()
        fresh.close()


# ---------------------------------------------------------------------------------------
# the L2 bound at norms far from 1 (regression: |q| |v| was taken as sqrt(|q|^2 |v|^2), whose argument underflows to 0 from norms
# of 1e-10 down and overflows from 1e10 up, where |q|^2 + |v|^2 -- the f32 path -- is still exact)
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale_log2", [-45, 45])
def test_screen_is_invariant_under_a_power_of_two_scale(pqv, monkeypatch, edge, scale_log2):
    """Rows and queries times 2^s: every f32 product and sum of the exact passes scales exactly, the normalised images do not change,
    so the rows are those of the unscaled corpus (checked against the reference) and the distances are its distances times 2^2s
    (L2) or its distances (cosine), bit for bit.  A screen bound that loses the norms' scale drops rows here."""
    corpus, ref = edge
    s = np.float32(2.0) ** np.float32(scale_log2)
    scaled = pqv.Corpus.upload(ref(br.COS).data * s)
    try:
        for metric in (br.COS, br.L2):
            r = ref(metric).take(slice(0, 130))
            for op in ("i8", "f16"):
                base = _call(pqv, monkeypatch, corpus, r.queries, K, metric, op)
                br.check(r, K, *base, what=f"{metric} {op}")
                got = _call(pqv, monkeypatch, scaled, r.queries * s, K, metric, op)
                want = base[1] * (s * s) if metric == br.L2 else base[1]
                br.assert_same_bits((base[0], want, base[2]), got, f"{metric} {op}: scaled by 2^{scale_log2}")
    finally:
        scaled.close()


# ---------------------------------------------------------------------------------------
# e. switches that are read once per process
# ---------------------------------------------------------------------------------------
_SWITCH_SCRIPT = r"""
import sys, os, hashlib
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np
import pq_vector_amd as pqv
import brute_ref as br
h = hashlib.sha256()
for kind, dim in (("normal", 160), ("uniform01", 256)):
    data, queries = br.make_case(kind, br.N_FORMS, dim, 300)
    corpus = pqv.Corpus.upload(data)
    for metric in (br.COS, br.L2):
        ref = br.reference(data, queries, 10, metric)
        for nq in (33, 130, 300):
            for op in ("i8", "f16"):
                os.environ["PQV_BRUTE_OP"] = op
                rows, dist, nf = corpus.brute_topk(queries[:nq], 10, pqv.PQV_COSINE if metric == br.COS else pqv.PQV_L2SQ_MFMA)
                br.check(ref.take(slice(0, nq)), 10, rows, dist, nf, what=f"{kind} {dim} {metric} nq {nq} {op}")
                h.update(rows.tobytes()); h.update(dist.tobytes()); h.update(nf.tobytes())
    corpus.close()
print("HASH", h.hexdigest())
"""


def _child(env):
    """runs the script under env; a non-zero return code fails the test at once with the child's stderr tail"""
    p = subprocess.run([sys.executable, "-c", _SWITCH_SCRIPT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return [l for l in p.stdout.splitlines() if l.startswith("HASH")][0]


def test_once_per_process_switches_never_change_a_result():
    """PQV_BRUTE_TILE and PQV_BRUTE_STAGE are read once per process: one child per setting runs both ops x both metrics x 33 / 130 /
    300 queries on two corpora, checks every answer against the reference itself and prints one hash of all rows and distance bits.
    TILE=128 is the only way the 128-query tile gets several query tiles (300 queries: ny = 3 in its XCD grid mapping), TILE=384 the
    256 x 128 tile, STAGE=64 the 256 x 256 tile's 64-byte stages at image rows of 256 and 512 bytes.  All hashes are equal.
    PQV_BRUTE_F16=0 scores every row with the first range's f32 kernel: checked against the reference, its bits are its own."""
    switches = [{}, {"PQV_BRUTE_TILE": "128"}, {"PQV_BRUTE_TILE": "256"}, {"PQV_BRUTE_TILE": "384"}, {"PQV_BRUTE_STAGE": "64"},
                {"PQV_BRUTE_TILE": "384", "PQV_BRUTE_STAGE": "64"}]
    base = dict(os.environ)
    for name in ("PQV_BRUTE_TILE", "PQV_BRUTE_STAGE", "PQV_BRUTE_F16", "PQV_BRUTE_RING", "PQV_BRUTE_STATS"):
        base.pop(name, None)
    got = [_child(dict(base, **sw)) for sw in switches]
    assert len(set(got)) == 1, list(zip(switches, got))
    _child(dict(base, PQV_BRUTE_F16="0"))
