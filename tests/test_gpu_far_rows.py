"""Every search and mutation path on rows beyond 2^31 / 2^32 bytes and elements of the caller's row matrix.

The workload is 10 M x 768 f32: every row past 5 592 405 starts beyond 2^32 elements, every row past 1 398 101 beyond 2^32 bytes.  A
16 GiB device buffer is only allocated and filled with a constant; the 4 608 rows of one case of tests/mutated_cases.py are written
around the four rows at which 32-bit address arithmetic breaks (tests/far_rows_cases.py: the map R), and Corpus.from_device_ptr adopts
the buffer.  The index stays tiny, and every exact-evaluation read of every mode -- the streaming kernels of stream_walk.hpp through
d_row_of, the assignment kernels of an append, rows_gather_kernel of a compact, normalize_rows_kernel of the first cosine call,
predicate_rows_kernel and mask_gather_kernel over 5.6 M row ids, fetch_rows -- lands where the benchmark's rows are.

Nothing expected comes from the library: the index states are held to the blobs of the numpy models (append_ref / remove_ref) with
their lists mapped through R, every call to mutated_cases.expect() on the DENSE model with its rows mapped through R, bit for bit,
the partition calls to partition_ref / partition_group_ref likewise.  A filler row (0.5 everywhere) is nearer to every uniform query
than any real row, carries every mask bit and query 0's keys: a read that lands on one changes an answer.
tests/test_far_rows_host.py holds the relocation to its premises."""
import time

import numpy as np
import pytest

import assign_exact
import distinct_filter_ref
import far_rows_cases as frc
import mutated_cases as mc
import partition_group_ref as pgr
import partition_ref as pr
import remove_ref
from mode_calls import GROUPS, METRIC, Handles, group_of, run
from test_gpu_partition import _host_filter, _same, part_device
from test_gpu_partition_grouped import grouped_device

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

NAME, TIES = "far768", "far768i"
FILL = 0.5
NEED_FREE = 40 << 30          # the buffer, one normalised copy of it behind the first cosine call, and room to work in
PRED_TS = mc.TS0 + 1000       # the predicate mask: ts >= PRED_TS (a NULL ts never passes)
LAYOUTS = ["images_only", "row_order"]
COPY_MODES = ["topk", "topk_device", "topk_masked", "range", "distinct", "dot"]


class FarCorpus:
    """One case on the GPU: the 16 GiB buffer with X at rows R, adopted as a corpus; the index states, made by the library"""

    def __init__(self, pqv, oracle, name):
        import torch
        free, total = torch.cuda.mem_get_info()
        if free < NEED_FREE:
            pytest.skip(f"the far corpus and one cosine copy of it need {NEED_FREE >> 30} GiB of device memory: {free} bytes free of {total}")
        self.pqv, self.oracle, self.name = pqv, oracle, name
        self.far = far = frc.far_case(oracle, name)
        self.case = c = far.case
        t0 = time.perf_counter()
        self.tensor = torch.empty((far.n_far, c.dim), dtype=torch.float32, device="cuda")
        self.tensor.fill_(FILL)
        self.tensor[torch.from_numpy(far.R).to("cuda")] = torch.from_numpy(c.X).to("cuda")
        torch.cuda.synchronize()
        assert self.tensor.is_contiguous() and self.tensor.numel() > 1 << 32
        self.corpus = pqv.Corpus.from_device_ptr(self.tensor.data_ptr(), far.n_far, c.dim, keepalive=self.tensor)
        print(f"{name}: {far.n_far} rows, {self.tensor.numel() * 4 / 2 ** 30:.2f} GiB allocated, filled and adopted in {time.perf_counter() - t0:.2f} s")
        self.index, self.dense, self.old_row = {}, None, None
        self.handles, self.layout, self.parts = None, None, {}
        self._memo = {}

    # ---- the states, each derived from the one before by the library ------------------------------------------------------------
    def make_states(self):
        if self.index:
            return self.index
        import torch
        pqv, far, c = self.pqv, self.far, self.case
        ix = self.index
        ix["built"] = pqv.Index.from_parts(c.dim, c.C, far.lists(c.models["built"].lists))
        ix["appended"] = ix["built"].append(self.corpus, first_row=int(far.R[c.n0]), n_rows=c.n1 - c.n0)
        self.flags = np.zeros(far.n_far, np.uint8)          # the dense flags at rows R; no filler row is flagged
        self.flags[far.R[:c.n1]] = c.flags
        ix["removed"] = ix["appended"].remove(flags=self.flags)
        ix["removed_device_flags"] = ix["appended"].remove(flags=torch.from_numpy(self.flags).to("cuda"))
        ix["grown"] = ix["removed"].append(self.corpus, first_row=int(far.R[c.n1]), n_rows=c.n2 - c.n1)
        ix["chained"] = ix["grown"].remove(far.rows(c.gone))          # (the two unindexed ids of `gone` stay what they are)
        self.dense, ix["compacted"], self.old_row = ix["chained"].compact(self.corpus)
        return ix

    # ---- one searcher at a time, with its masks, keys and columns ----------------------------------------------------------------
    def searcher(self, layout):
        """Handles of the `chained` far index in `layout`; the handles of another layout are closed first"""
        from pq_vector_amd import _ffi
        if self.layout != layout:
            self.close_handles()
            index = self.make_states()["chained"]
            flags = _ffi.PQV_LAYOUT_ROW_ORDER if layout == "row_order" else _ffi.PQV_LAYOUT_IVF_ORDERED
            s = self.pqv.Searcher(index, self.corpus, flags)
            fp = s.footprint()
            listed = sum(len(l) for l in self.case.models["chained"].lists)
            if layout == "copy":            # a list-ordered f32 copy of the listed rows, gathered from the far rows
                assert fp["ivf_rows_bytes"] == listed * self.case.dim * 4, fp
            else:                           # the caller's matrix, rows found through the list order
                assert fp["ivf_rows_bytes"] == 0 and fp["row_order_bytes"] == self.far.n_far * self.case.dim * 4, fp
                assert (fp["blocked_bytes"] > 0) == (layout == "images_only"), fp
            self.handles, self.layout = Handles(self.pqv, self.far.model("chained"), s), layout
        return self.handles

    def close_handles(self):
        for p in self.parts.values():          # (the key partitions of the searcher that goes)
            p.close()
        self.parts = {}
        if self.handles is not None:
            self.handles.close()
        self.handles = self.layout = None

    def modes(self, group=None):
        dense = self.case.models["chained"]
        if "modes" not in self._memo:
            self._memo["modes"] = {n: mc.resolve(self.oracle, dense, sp) for n, sp in mc.modes(self.name).items()}
        return {n: sp for n, sp in self._memo["modes"].items() if group is None or group_of(sp) == group}

    def expect(self, mode):
        """mutated_cases.expect() on the dense `chained` model, its rows through R"""
        if mode not in self._memo:
            self._memo[mode] = self.far.relocate(mc.expect(self.oracle, self.case.models["chained"], self.modes()[mode]))
        return self._memo[mode]

    def close(self):
        self.close_handles()
        for ix in self.index.values():
            ix.close()
        if self.dense is not None:
            self.dense.close()
        self.corpus.close()
        self.tensor = None


class World:
    """At most one far corpus at a time"""

    def __init__(self, pqv, oracle):
        self.pqv, self.oracle, self.now = pqv, oracle, None

    def get(self, name):
        if self.now is not None and self.now.name != name:
            self.close()
        if self.now is None:
            self.now = FarCorpus(self.pqv, self.oracle, name)
        return self.now

    def close(self):
        import torch
        if self.now is not None:
            self.now.close()
            self.now = None
            torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def world(pqv, oracle):
    import torch
    torch.cuda.reset_peak_memory_stats()
    w = World(pqv, oracle)
    yield w
    w.close()


def _route(h, layout, metric="l2", nq=32):
    """as tests/test_gpu_mutated_search.py's: the wide screen with int8 operands (768 dims, the images-only layout), the exact
    stream for PQV_DOT; the row-order layout has no operand images"""
    plan = h.s.describe(nq, mc.K, mc.NPROBE, METRIC[metric])
    if metric == "dot":
        assert "dot_stream_kernel" in plan, plan
    elif layout == "images_only":
        assert "wide_filter_kernel" in plan and (metric != "l2" or "int8 screen operands" in plan), plan
    else:
        assert "wide_filter_kernel" not in plan, plan
    return plan


# ---- a. mutations at far rows, made by the library -----------------------------------------------------------------------------------
def test_fetch_rows_across_every_run(world):
    w = world.get(NAME)
    far, c = w.far, w.case
    edges = [0, 767, 768, 1535, 1536, 2303, 2304, 3071, c.n0, c.n1 - 1, c.n1, c.n2 - 1]
    at_breaks = [int(np.searchsorted(far.R, b)) + d for b in far.breaks for d in (-1, 0, 1)]
    ids = np.array(edges + at_breaks + list(np.random.default_rng(1).permutation(c.n2)[:200]), np.int64)
    assert all((far.R[at_breaks[3 * i + 1]] == b) for i, b in enumerate(far.breaks))
    got = w.corpus.fetch_rows(far.R[ids].astype(np.uint32))
    assert np.array_equal(got.view(np.uint32), c.X[ids].view(np.uint32))
    filler = w.corpus.fetch_rows(np.array([768, far.breaks[3] + 600, far.n_far - 513], np.uint32))          # (rows of no run)
    assert (filler == np.float32(FILL)).all()


def test_mutations_at_far_rows(world, pqv, oracle):
    from pq_vector_amd import _ffi
    w = world.get(NAME)
    far, c = w.far, w.case
    # Index.assign over the first appended range: append_ref's assignment (the exact nearest centroid)
    built = pqv.Index.from_parts(c.dim, c.C, far.lists(c.models["built"].lists))
    got = built.assign(w.corpus, first_row=int(far.R[c.n0]), n_rows=c.n1 - c.n0)
    assert np.array_equal(got, assign_exact.nearest(c.X[c.n0:c.n1], c.C)[0].astype(np.uint32))
    got = built.assign(w.corpus, first_row=int(far.R[c.n1]), n_rows=c.n2 - c.n1)
    assert np.array_equal(got, assign_exact.nearest(c.X[c.n1:], c.C)[0].astype(np.uint32))
    built.close()

    ix = w.make_states()
    want = {s: c.models[s].lists for s in ("built", "appended", "removed", "chained")}
    want["grown"], want["removed_device_flags"] = c.grown, c.models["removed"].lists
    bound = {"built": c.n0, "appended": c.n1, "removed": c.n1, "removed_device_flags": c.n1, "grown": c.n2, "chained": c.n2}
    assert far.bound(c.n1) == far.R[c.n0] + (c.n1 - c.n0) and far.bound(c.n2) == far.n_far
    for state, lists in want.items():
        assert ix[state].to_bytes() == remove_ref.blob(oracle, c.dim, c.C, far.lists(lists)), f"the lists of {state} are not the model's, relocated"
        assert ix[state].n_rows == sum(len(l) for l in lists), state
        assert ix[state].row_bound == far.bound(bound[state]) == _ffi.lib().pqv_index_row_bound(ix[state]._h), state
    assert ix["removed"].to_bytes() == ix["removed_device_flags"].to_bytes()          # flags as a numpy array and as a CUDA tensor

    # compacted: the dense corpus' rows are the model's, bit for bit, and so are its index and old_row
    m = c.models["compacted"]
    assert np.array_equal(w.old_row, far.rows(c.old_row)) and w.dense.rows == m.n == len(c.old_row)
    back = w.dense.fetch_rows(np.arange(m.n, dtype=np.uint32))
    assert np.array_equal(back.view(np.uint32), m.X.view(np.uint32))
    assert ix["compacted"].to_bytes() == remove_ref.blob(oracle, c.dim, c.C, m.lists) and ix["compacted"].row_bound == m.bound


# ---- d. key partitions at far rows (on the images-only searcher, before its first cosine call) --------------------------------------
def _flt(c, name, nq):
    """a filter of the case as tests/test_gpu_partition.py passes one: (name, kind, a, b) of plain integers"""
    col, kind, spec = c.filter_of(name, nq)
    _, a, b = distinct_filter_ref.descriptor(kind, spec)
    return col, (name, kind, [int(x) for x in a], None if b is None else [int(x) for x in b])


def _partitions(w, h):
    """-> ({column: the searcher's KeyPartition}, {column: the restatement's partition over the DENSE rows})"""
    fm, dense = w.far.model("chained"), w.case.models["chained"]
    if not w.parts:
        tenant = w.pqv.Column.upload(fm.cols["tenant"][0])
        w.parts = {"tenant": h.s.key_partition(tenant), "ts": h.s.key_partition("ts")}          # (ts: the attached column, with NULLs)
        tenant.close()
    if "parts" not in w._memo:
        indexed = np.nonzero(dense.in_lists())[0]
        w._memo["parts"] = {col: pr.build(dense.cols[col][0], dense.cols[col][1], indexed) for col in w.parts}
    return w.parts, w._memo["parts"]


@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_key_partitions_at_far_rows(world, metric):
    w = world.get(NAME)
    far, c, dense = w.far, w.case, w.case.models["chained"]
    h = w.searcher("images_only")
    parts, ref = _partitions(w, h)
    d = pr.distances(metric, pr.REF4, c.X, c.Q)
    for col, (prows, pkeys) in ref.items():
        assert parts[col].rows == len(prows) > 0
        _same(parts[col].keys(), pr.distinct(pkeys), f"keys() of {col}")
    for fname in ("eq", "in", "range"):
        col, flt = _flt(c, fname, len(c.Q))
        prows, pkeys = ref[col]
        for allow, mask in ((None, None), (dense.masks["dense"], h.masks["dense"])):
            what = f"{metric} {fname} {'masked' if mask else 'plain'}"
            exp = list(pr.topk_batch(prows, pkeys, flt[1], flt[2], flt[3], d, mc.K, metric, False, allow)[:4])
            assert (exp[2] > 0).sum() >= len(c.Q) // 2, what
            exp[0] = far.rows(exp[0])
            _same(part_device(h.s, parts[col], c.Q, mc.K, flt, mask=mask, metric=METRIC[metric]), exp, what + ": device form")
            host = h.s.topk_partition(c.Q, mc.K, parts[col], mask=mask, metric=METRIC[metric], sqrt_out=False, **_host_filter(flt))
            _same(host, exp, what + ": host form")


@pytest.mark.parametrize("m", [3, 1])
def test_grouped_key_partitions_at_far_rows(world, m):
    w = world.get(NAME)
    far, c, dense = w.far, w.case, w.case.models["chained"]
    h = w.searcher("images_only")
    parts, ref = _partitions(w, h)
    d = pr.distances("l2", pr.REF4, c.X, c.Q)
    doc, doc_valid = dense.cols["doc"]
    for fname in ("eq", "in", "range"):
        col, flt = _flt(c, fname, len(c.Q))
        prows, pkeys = ref[col]
        for allow, mask in ((None, None), (dense.masks["dense"], h.masks["dense"])):
            what = f"grouped m={m} {fname} {'masked' if mask else 'plain'}"
            exp = list(pgr.grouped_batch(prows, pkeys, flt[1], flt[2], flt[3], d, doc, doc_valid, mc.K, m, "l2", False, allow)[:6])
            assert (exp[4] > 0).sum() >= len(c.Q) // 2, what
            exp[0] = far.rows(exp[0])
            _same(grouped_device(h.s, parts[col], h.keys["doc"], c.Q, mc.K, m, flt, mask=mask), exp, what + ": device form")
            host = h.s.topk_partition_grouped(c.Q, mc.K, m, parts[col], h.keys["doc"], mask=mask, sqrt_out=False, **_host_filter(flt))
            _same(host, exp, what + ": host form")


# ---- row masks and the predicate mask over 5.6 M row ids -------------------------------------------------------------------------------
def test_row_masks_keep_the_callers_bytes_and_count_list_rows(world, pqv, oracle):
    w = world.get(NAME)
    h = w.searcher("images_only")
    fm, dense = w.far.model("chained"), w.case.models["chained"]
    inside = fm.in_lists()
    for mask_name, mask in h.masks.items():
        a = h.mask_bytes[mask_name]
        assert mask.rows == h.n == len(a) == w.far.n_far
        assert np.array_equal(mask.to_bytes(), a.astype(np.uint8)), mask_name          # filler and removed rows included
        assert mask.count == int((a & inside).sum()), mask_name
    # a predicate over the attached column (int64 with NULLs, one value per row of the big corpus): the mask the same bytes make
    pred = h.s.row_mask(pqv.col("ts") >= PRED_TS)
    ts, valid = fm.cols["ts"]
    want = valid & (ts >= PRED_TS)
    assert np.array_equal(pred.to_bytes(), want.astype(np.uint8)) and pred.count == int((want & inside).sum())
    assert 0 < pred.count < int(inside.sum())
    by_bytes = h.s.row_mask(want)
    want_dense = want[w.far.R]
    assert np.array_equal(want_dense, dense.cols["ts"][1] & (dense.cols["ts"][0] >= PRED_TS))
    for sp in (mc.spec("topk", mask=want_dense), mc.spec("topk_device", mask=want_dense, nprobe=w.case.nprobe_f), dict(w.modes()["range_masked"], mask=want_dense)):
        got = run(h, sp, mask=pred)
        mc.same(got, w.far.relocate(mc.expect(oracle, dense, sp)), what=f"{NAME} chained predicate mask {sp['call']}")
        mc.same(run(h, sp, mask=by_bytes), got, what=f"{NAME} chained predicate mask against its bytes")
    pred.close()
    by_bytes.close()


# ---- b. every mode on the `chained` far index, in the two layouts that read the caller's matrix ------------------------------------------
@pytest.mark.parametrize("layout,group", [(l, g) for l in LAYOUTS for g in GROUPS])
def test_mode_equals_the_references_at_far_rows(world, layout, group):
    """(the cosine modes on the images-only layout alone: a searcher that has answered one holds a normalised copy of the 16 GiB)"""
    import torch
    w = world.get(NAME)
    h = w.searcher(layout)
    _route(h, layout)
    modes = {n: sp for n, sp in w.modes(group).items() if sp["metric"] != "cos" or layout == "images_only"}
    assert modes
    for mode, sp in modes.items():
        mc.same(run(h, sp), w.expect(mode), what=f"{NAME} chained {layout} {mode}")
        if sp["metric"] != "l2":
            _route(h, layout, sp["metric"])          # (after the call: a first cosine call makes the searcher describe() speaks of)
    if group == "metrics":
        fp = h.s.footprint()
        assert (fp["row_order_bytes"] == 2 * w.far.n_far * w.case.dim * 4) == (layout == "images_only"), fp          # the cosine copy
        print(f"{layout}: max_memory_allocated {torch.cuda.max_memory_allocated()} bytes, searcher footprint {fp}")


# ---- c. the copying layout ---------------------------------------------------------------------------------------------------------------
def test_the_copying_layout_gathers_far_rows(world, monkeypatch):
    monkeypatch.setenv("PQV_IVF_COPY", "1")          # (read when the searcher is made)
    w = world.get(NAME)
    h = w.searcher("copy")
    plan = h.s.describe(32, mc.K, mc.NPROBE, METRIC["l2"])
    assert "wide_filter_kernel" in plan and "int8 screen operands" in plan, plan
    for mode in COPY_MODES:
        mc.same(run(h, w.modes()[mode]), w.expect(mode), what=f"{NAME} chained copy {mode}")
    w.close_handles()


# ---- e. ties at far rows -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", ["plain", "masks"])
def test_ties_at_far_rows(world, group):
    """integer data: the kth place ties, and pqv_topk's heap replays -- which fetch the tied rows from the far corpus -- run"""
    w = world.get(TIES)          # (the first far corpus is freed before this one is made)
    h = w.searcher("images_only")
    _route(h, "images_only")
    modes = w.modes(group)
    assert modes and ("topk" in modes) == (group == "plain")
    for mode, sp in modes.items():
        before = h.s.counters()["exact_replays"]
        mc.same(run(h, sp), w.expect(mode), what=f"{TIES} chained {mode}")
        assert mode != "topk" or h.s.counters()["exact_replays"] > before          # (as test_ties_replay_the_heap: the oracle's heap order)
