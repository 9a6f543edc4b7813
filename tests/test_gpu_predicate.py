"""Predicate masks on the GPU (pqv_column_*, pqv_row_mask_from_predicates, pqv_row_mask_to_bytes).

Truth is held to tests/predicate_ref.py -- the numpy evaluation of the compiled program and, independently, pyarrow's evaluation
of the translated tree (test_predicate_host.py pins the two to each other); searches are held to the byte-made mask of the same
truth, bit for bit, which tests/test_gpu_mask.py holds to the filtered-lists setup and the oracle."""
import json
import os
import threading

import numpy as np
import pytest

import predicate_ref as ref
from test_gpu_mask import Setup, _device, _same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Rows:
    """n rows of dim 8 in 8 hand-made lists (about 5 % of the rows in none), the typed columns of predicate_ref attached."""

    def __init__(self, pqv, n, seed):
        rng = np.random.default_rng(seed)
        self.pqv, self.n = pqv, n
        self.data = rng.random((n, 8), dtype=np.float32)
        listed = np.flatnonzero(rng.random(n) >= 0.05)
        rng.shuffle(listed)
        self.lists = [np.sort(part).astype(np.uint32) for part in np.array_split(listed, 8)]
        self.listed = np.zeros(n, bool)
        self.listed[listed] = True
        self.corpus = pqv.Corpus.upload(self.data)
        self.s = pqv.Searcher(pqv.Index.from_parts(8, rng.random((8, 8), dtype=np.float32), self.lists), self.corpus)
        self.columns = ref.make_columns(n, seed + 1)
        self.dtypes = ref.dtypes_of(self.columns)
        for name, (values, valid) in self.columns.items():
            c = self.s.attach_column(name, pqv.Column.upload(values, valid))
            assert c.rows == n and c.dtype == self.dtypes[name] and c.device == 0

    def check(self, p, want, what):
        m = self.s.row_mask(p)
        try:
            got = m.to_bytes()
            assert got.dtype == np.uint8 and got.shape == (self.n,)
            assert (got == want).all(), (what, np.flatnonzero(got != want)[:8])
            assert m.rows == self.n and m.count == int(want[self.listed].sum()), what
        finally:
            m.close()


@pytest.fixture(scope="module")
def rows(pqv):
    return Rows(pqv, 4099, seed=31)


def _operands(name, values, count):
    """operands worth comparing a column against: its extremes and awkward values first, then a few of its own values"""
    special = {"i32": [0, 2**31 - 1, -2**31, 2**40], "i64": [2**53, 2**53 + 1, 2**32 + 7, 0],
               "f32": [0.0, float("nan"), float("inf"), -0.5], "f64": [0.0, float("nan"), float("-inf"), 0.1], "plain": [2, 0, -1, 3]}[name]
    return special[:count]


def _leaves_of(pqv, name, a, b):
    c = pqv.col(name)
    return {"EQ": c == a, "NE": c != a, "LT": c < a, "LE": c <= a, "GT": c > a, "GE": c >= a, "BETWEEN": c.between(a, b),
            "IS_NULL": c.is_null()}


def _truth_tables(r, n_operands):
    pqv = r.pqv
    for name, (values, valid) in r.columns.items():
        ops = _operands(name, values, n_operands)
        for i, a in enumerate(ops):
            b = ops[(i + 1) % len(ops)] if len(ops) > 1 else a
            if a == a and b == b and a > b:
                a, b = b, a
            for opname, leaf in _leaves_of(pqv, name, a, b).items():
                for negate in (False, True):
                    p = ~leaf if negate else leaf
                    comp = p.compile(r.dtypes)
                    assert len(comp.leaves) == 1 and bool(comp.ops[0] & 0x100) == negate
                    r.check(p, ref.evaluate(comp, r.columns), f"{name} {opname} {a!r} {b!r} negate={negate}")


def test_truth_tables_every_op_negation_and_type(rows):
    """Case 1: every op x negate x dtype (NULLs, NaN, +-inf, -0.0, 2^53 against 2^53 + 1, a column without validity)."""
    _truth_tables(rows, 4)
    # what the contract spells out, by value
    pqv, c = rows.pqv, rows.columns
    i64, ok = c["i64"][0], c["i64"][1] != 0
    assert ((i64 == 2**53) & ok).any() and ((i64 == 2**53 + 1) & ok).any()
    rows.check(pqv.col("i64") == 2**53, ((i64 == 2**53) & ok).astype(np.uint8), "2^53 stays distinct from 2^53 + 1")
    rows.check(pqv.col("i64") > 2**53, ((i64 > 2**53) & ok).astype(np.uint8), "beyond 2^53")
    f64, okf = c["f64"][0], c["f64"][1] != 0
    assert (np.isnan(f64) & okf).any() and ((f64 == 0) & np.signbit(f64) & okf).any()
    rows.check(~(pqv.col("f64") < 0.0), (okf & ~(f64 < 0.0)).astype(np.uint8), "a negated LT is true on NaN")
    rows.check(pqv.col("f64") == 0.0, (okf & (f64 == 0.0)).astype(np.uint8), "-0.0 == 0.0")
    rows.check(pqv.col("f64") != 1.0, (okf & ((f64 != 1.0) | np.isnan(f64))).astype(np.uint8), "NE is true on NaN")
    rows.check(pqv.col("plain").is_null(), np.zeros(rows.n, np.uint8), "a column without validity is never NULL")
    rows.check(pqv.col("i32") == 2**40, np.zeros(rows.n, np.uint8), "an operand beyond int32 never matches")


@pytest.mark.parametrize("n", [37, 64, 128])
def test_truth_tables_at_word_edges(pqv, n):
    """Case 1, continued: fewer rows than a word, exactly one word, exactly two."""
    _truth_tables(Rows(pqv, n, seed=40 + n), 1)


def test_random_trees_equal_both_references(rows):
    """Case 2: 200 seeded random trees of depth <= 4; a 32-leaf program; a right-nested program of depth 32."""
    table = ref.arrow_table(rows.columns)
    n_true = 0
    for p, comp in ref.compilable_trees(200, rows.columns, depth=4, seed=77):
        want = ref.evaluate(comp, rows.columns)
        assert (want == ref.evaluate_arrow(p, rows.columns, table)).all()
        rows.check(p, want, comp)
        n_true += int(want.sum())
    assert 0 < n_true < 200 * rows.n
    c = rows.pqv.col
    wide = c("i32").isin(range(-5, 6)) | c("i64").isin(range(-5, 6)) | c("f64").isin([0.25 * i for i in range(10)])
    comp = wide.compile(rows.dtypes)
    assert len(comp.leaves) == 32 and len(comp.program) == 63
    rows.check(wide, ref.evaluate(comp, rows.columns), "32 leaves")
    assert (ref.evaluate(comp, rows.columns) == ref.evaluate_arrow(wide, rows.columns, table)).all()
    deep = c("i32") == 15
    for i in range(30, -1, -1):                     # leaf 0 | (leaf 1 | (... | leaf 31)): all 32 pushed before the first OR
        deep = (c("i32") == i - 16) | deep
    comp = deep.compile(rows.dtypes)
    depth = np.cumsum([-1 if b >= 0x80 else 1 for b in comp.program]).max()
    assert depth == 32 and len(comp.program) == 63 and len(comp.leaves) == 32
    rows.check(deep, ref.evaluate(comp, rows.columns), "depth 32")
    assert (ref.evaluate(comp, rows.columns) == ref.evaluate_arrow(deep, rows.columns, table)).all()


def test_mask_leaves(rows):
    """Case 3: a byte-made mask AND a predicate; a negated mask; a predicate mask as a leaf of another; another searcher's mask."""
    pqv, s = rows.pqv, rows.s
    rng = np.random.default_rng(5)
    bytes_ = (rng.random(rows.n) < 0.5).astype(np.uint8)
    bm = s.row_mask(bytes_)
    assert (bm.to_bytes() == bytes_).all()
    odd = (rng.integers(0, 3, rows.n) * 7).astype(np.uint8)              # nonzero = allowed: to_bytes says 1
    om = s.row_mask(odd)
    assert (om.to_bytes() == (odd != 0)).all()
    om.close()
    p = pqv.col("i32") >= 0
    t = ref.evaluate(p.compile(rows.dtypes), rows.columns)
    rows.check(pqv.allowed(bm) & p, bytes_ & t, "mask AND predicate")
    rows.check(~pqv.allowed(bm), 1 - bytes_, "negated mask")
    rows.check(~(pqv.allowed(bm) | p), (1 - bytes_) & ref.evaluate((~p).compile(rows.dtypes), rows.columns), "De Morgan over a mask leaf")
    comp = (pqv.allowed(bm) & p).compile(rows.dtypes)
    assert (ref.evaluate(comp, rows.columns, {id(bm): bytes_}) == (bytes_ & t)).all()
    pm = s.row_mask(p)
    q = pqv.col("f64").is_null() | (pqv.col("plain") == 2)
    tq = ref.evaluate(q.compile(rows.dtypes), rows.columns)
    rows.check(pqv.allowed(pm) & ~q, t & (1 - tq), "a predicate mask as a leaf")
    rows.check(pqv.allowed(pm) | pqv.allowed(bm), t | bytes_, "two mask leaves")
    other = pqv.Searcher(pqv.Index.from_parts(8, np.zeros((8, 8), np.float32), rows.lists), rows.corpus)
    foreign = other.row_mask(bytes_)
    with pytest.raises(pqv.PqvError, match="row mask belongs to another searcher") as e:
        s.row_mask(pqv.allowed(foreign) & p)
    assert e.value.code == -1
    # the column checks of the library
    short = pqv.Column.upload(np.zeros(rows.n - 1, np.int32))
    s.attach_column("short", short)
    with pytest.raises(pqv.PqvError, match=f"column has {rows.n - 1} rows, the corpus has {rows.n}"):
        s.row_mask(pqv.col("short") == 0)
    del s.columns["short"]
    with pytest.raises(pqv.PqvError, match="no column named 'nope'"):
        s.row_mask(pqv.col("nope") == 0)
    with pytest.raises(pqv.PqvError, match=f"column has 3 rows, the corpus has {rows.n}"):
        s.attach_column("three", np.zeros(3, np.int64))
    for m in (bm, pm, foreign):
        m.close()
    other.close()


def _searches(st, m, metric, with_device=True):
    """every masked entry point with mask m -> (results, counter deltas)"""
    pqv, q = st.pqv, st.queries
    before = st.s.counters()
    out = []
    for nprobe in (1, 4, st.kc):
        for k in (1, 10):
            out.append(st.s.topk(q, k, nprobe, metric=metric, mask=m))
            if with_device:
                for flags in (False, True):
                    got = _device(st.s, q, k, nprobe, flags, mask=m, metric=metric)
                    out.append(got if flags else got[:4])
        out.append(st.s.range_search(q, st.radius_of[(nprobe, metric)], nprobe, metric=metric, mask=m))
    out.append(st.s.topk(q[:2], 1100, 2, metric=metric, mask=m))                     # k > 1024: the host heap
    after = st.s.counters()
    return out, {key: after[key] - before[key] for key in ("embeddings_fetched", "candidate_rows", "exact_replays", "queries")}


@pytest.mark.parametrize("dim", [30, 64])
@pytest.mark.parametrize("layout", ["ivf", "row"])
def test_searches_equal_the_byte_made_mask(pqv, oracle, dim, layout):
    """Case 4: integer-valued data (ties: the heap replay reads the lazily fetched host bytes), both layouts, REF4 and COSINE."""
    flags = pqv.PQV_LAYOUT_IVF_ORDERED if layout == "ivf" else pqv.PQV_LAYOUT_ROW_ORDER
    st = Setup(pqv, oracle, 3000, dim, 6, seed=50 + dim, integer=True, flags=flags)
    columns = ref.make_columns(st.n, seed=9)
    for name, (values, valid) in columns.items():
        st.s.attach_column(name, pqv.Column.upload(values, valid))
    p = ((pqv.col("i32") >= 0) | pqv.col("f32").between(-1.0, 1.5)) & ~pqv.col("i64").is_null()
    truth = ref.evaluate(p.compile(ref.dtypes_of(columns)), columns)
    assert 0.2 < truth.mean() < 0.8
    st.radius_of = {(nprobe, metric): st.radius(nprobe, metric) for nprobe in (1, 4, st.kc) for metric in (pqv.PQV_L2SQ_REF4, pqv.PQV_COSINE)}
    for metric in (pqv.PQV_L2SQ_REF4, pqv.PQV_COSINE):
        bm = st.s.row_mask(truth.astype(bool))
        pm = st.s.row_mask(p)                          # fresh: its host bytes are fetched inside the first tie replay
        assert pm.count == bm.count
        exp, exp_counts = _searches(st, bm, metric)
        got, got_counts = _searches(st, pm, metric)
        assert len(got) == len(exp)
        for i, (g, e) in enumerate(zip(got, exp)):
            _same(g, e, f"call {i} metric {metric}")
        assert got_counts == exp_counts and exp_counts["exact_replays"] > 0 and exp_counts["embeddings_fetched"] > 0
        assert (pm.to_bytes() == truth).all()
        bm.close(); pm.close()


def test_lazy_host_bytes_under_threads(pqv, oracle):
    """Case 5: four threads run the tie-heavy topk at once on a fresh predicate mask; four more race to_bytes on another."""
    st = Setup(pqv, oracle, 3000, 8, 6, seed=4, integer=True)
    values = np.random.default_rng(3).integers(0, 8, st.n).astype(np.int32)
    st.s.attach_column("v", values)
    p = pqv.col("v") < 4
    truth = (values < 4).astype(np.uint8)
    q = np.random.default_rng(2).integers(0, 3, (24, 8)).astype(np.float32)
    bm = st.s.row_mask(truth)
    before = st.s.counters()["exact_replays"]
    exp = st.s.topk(q, 20, st.kc, mask=bm)
    assert st.s.counters()["exact_replays"] > before
    for job in ("topk", "to_bytes"):
        pm = st.s.row_mask(p)
        results, errors = [None] * 4, []
        start = threading.Barrier(4)

        def run(i):
            try:
                start.wait()
                results[i] = st.s.topk(q, 20, st.kc, mask=pm) if job == "topk" else pm.to_bytes()
            except Exception as e:      # noqa: BLE001 -- reported below
                errors.append(e)
        threads = [threading.Thread(target=run, args=(i,)) for i in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        for r in results:
            if job == "topk":
                _same(r, exp, "threaded topk")
            else:
                assert (r == truth).all()
        pm.close()
    bm.close()


def test_table_searcher_with_a_corpus_aligned_column(pqv, oracle):
    """Case 6: two files with a gap between their row ranges; row r of the column is corpus row r."""
    from test_gpu_table import Table
    rng = np.random.default_rng(12)
    t = Table(pqv, oracle, rng, [900, 1400], [4, 6], 32, gap=5)
    n = len(t.data)
    assert n > 2300                                                 # (the gap rows belong to no file)
    values = rng.integers(0, 10, n).astype(np.int64)
    valid = (rng.random(n) > 0.1).astype(np.uint8)
    t.s.attach_column("v", pqv.Column.upload(values, valid))
    p = pqv.col("v") < 4
    truth = ((values < 4) & (valid != 0)).astype(np.uint8)
    pm, bm = t.s.row_mask(p), t.s.row_mask(truth)
    assert pm.rows == n and pm.count == bm.count and (pm.to_bytes() == truth).all()
    queries = rng.random((4, 32), dtype=np.float32)
    for nprobe in (1, 2):
        _same(t.s.topk(queries, 10, nprobe, mask=pm), t.s.topk(queries, 10, nprobe, mask=bm), "table topk")
        _same(_device(t.s, queries, 10, nprobe, True, mask=pm), _device(t.s, queries, 10, nprobe, True, mask=bm), "table device")
        _same(t.s.range_search(queries, 2.0, nprobe, mask=pm), t.s.range_search(queries, 2.0, nprobe, mask=bm), "table range")
    pm.close(); bm.close()


@pytest.mark.parametrize("which", [0, 1])
def test_builders_reference_fixtures_and_the_column_cache(pqv, tmp_path, monkeypatch, which):
    """Case 7: the reference's two filtered integration tests through .where(pqv.col("id") >= n); all four builders; a second
    search on the same file loads no column again."""
    import pyarrow as pa
    import pyarrow.compute as pc
    import pyarrow.parquet as pq
    from pq_vector_amd import parquet_io
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_filter_fixtures.json")))["fixtures"][which]
    path = str(tmp_path / "t.parquet")
    vec = pa.array(fx["vectors"], type=pa.list_(pa.float32()))
    pq.write_table(pa.table({"id": pa.array(range(6), type=pa.int32()), "tag": pa.array(list("abcdef")), "vec": vec}), path)
    pqv.IndexBuilder(path, "vec").build_inplace()
    loads = []
    real = parquet_io.load_scalar_column
    monkeypatch.setattr(parquet_io, "load_scalar_column", lambda *a, **kw: (loads.append(a[1]), real(*a, **kw))[1])
    p = pqv.col("id") >= fx["id_ge"]
    s = pqv.searcher_for_parquet(path)
    assert "id" not in s.columns
    before = s.counters()
    res = pqv.TopkBuilder(path, [0, 0]).k(2).nprobe(64).where(p).search()
    after = s.counters()
    assert [r.row_idx for r in res] == fx["ids"]
    assert after["candidate_rows"] - before["candidate_rows"] == fx["candidate_rows"]
    assert after["embeddings_fetched"] - before["embeddings_fetched"] == fx["embeddings_fetched"]
    host = pqv.TopkBuilder(path, [0, 0]).k(2).nprobe(64).where(pc.field("id") >= fx["id_ge"]).search()
    assert [(r.row_idx, r.distance) for r in res] == [(r.row_idx, r.distance) for r in host]
    # the cache: the column was loaded once and stays with the cached searcher
    assert loads == ["id"] and pqv.searcher_for_parquet(path) is s
    column = s.columns["id"]
    assert column.rows == 6 and column.dtype == 0
    again = pqv.TopkBuilder(path, [0, 0]).k(2).nprobe(64).where(pqv.col("id") >= fx["id_ge"]).search()
    hits = pqv.RangeBuilder(path, [0, 0]).radius(100.0).nprobe(64).where(p).search()
    assert loads == ["id"] and s.columns["id"] is column
    assert [r.row_idx for r in again] == fx["ids"]
    assert sorted(r.row_idx for r in hits) == list(range(fx["id_ge"], 6)) and [r.row_idx for r in hits[:2]] == fx["ids"]
    # a table of the file twice: one corpus-row-aligned column
    tres = pqv.TableTopkBuilder([path, path], [0, 0]).k(2).nprobe(64).where(p).search()
    assert [r.row_idx for r in tres] == [fx["ids"][0], fx["ids"][0]]
    ts = pqv.searcher_for_parquet_files([path, path])
    tcol = ts.columns["id"]
    assert tcol.rows == 12
    tr = pqv.TableRangeBuilder([path, path], [0, 0]).radius(100.0).nprobe(64).where(p & (pqv.col("id") < 5)).search()
    assert sorted(r.row_idx for r in tr) == sorted(list(range(fx["id_ge"], 5)) * 2) and ts.columns["id"] is tcol
    same = pqv.TableTopkBuilder([path, path], [0, 0]).k(2).nprobe(64).where(pc.field("id") >= fx["id_ge"]).search()
    assert [(r.path, r.row_idx, r.distance) for r in tres] == [(r.path, r.row_idx, r.distance) for r in same]
    # a column that cannot be resident is refused by name, with the host route
    with pytest.raises(pqv.PqvError, match=r"column 'tag' has type string.*pyarrow expression"):
        pqv.TopkBuilder(path, [0, 0]).k(2).nprobe(64).where(pqv.col("tag") == 1).search()
    # a Searcher source resolves names against its attached columns
    assert [r.row_idx for r in pqv.TopkBuilder(s, [0, 0]).k(2).nprobe(64).where(p).search()] == fx["ids"]
