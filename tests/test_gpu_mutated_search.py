"""Every search mode on appended, removed and compacted indexes (include/pqv.h: "an unmasked search of the result returns what a
search of `index` under the equivalent pqv_row_mask returns -- through every fast path"; searchers made before the corpus grew
"keep working on the rows they have").

The states of tests/mutated_cases.py are made on the GPU the way a user makes them -- Corpus.create + append, IndexBuilder.build,
Index.append / remove(flags=) / remove(ids) / compact -- and each state's to_bytes() is held to the blob of the model's lists before
any search.  Every call is then compared, bit for bit, with mutated_cases.expect(): the numpy references over
oracle.index_from_parts(dim, C, the model's lists) and X.  Nothing expected comes from the library.  On top of that three relations
between the states hold for every mode: removed == appended under row_mask(~flags); compacted == chained through old_row; handles
made on `built` before the corpus grew answer as they did.  tests/test_mutated_cases_host.py holds the zoo to its premises."""
import numpy as np
import pytest

import mutated_cases as mc
import remove_ref
from mode_calls import GROUPS, METRIC, Handles, group_of, heap_order, run

pytestmark = pytest.mark.gpu

PRED_TS = mc.TS0 + 1000          # the predicate mask: ts >= PRED_TS (a NULL ts never passes)

# (int8_256 runs plain, cosine, masked and distinct only: a case is paired with the groups it has modes of)
CASE_GROUPS = [(n, g) for n in mc.CASES for g in GROUPS if any(group_of(sp) == g for sp in mc.modes(n).values())]


class Zoo:
    """One case on the GPU: the corpus that grows, the five indexes, a searcher with masks and keys for each."""

    def __init__(self, pqv, oracle, name, searchers=True):
        """searchers False: the corpus and the five indexes only (tests/test_gpu_mutated_table.py makes its own searchers)"""
        from pq_vector_amd import _ffi
        self.pqv, self.oracle, self.name = pqv, oracle, name
        self.h, self.old, self.under = {}, None, None
        self.case = c = mc.case(oracle, name)
        m, X = c.models, c.X
        self.corpus = corpus = pqv.Corpus.create(c.n2, c.dim)
        corpus.append(X[:c.n0])
        self.index = {"built": pqv.IndexBuilder(corpus).n_clusters(c.kc).max_iters(5).workers(1).build()}
        self._check_lists("built")
        # the handles of relation 3: a searcher, its masks and its keys made BEFORE the corpus grows, and what they answer now
        if searchers:
            self.old = Handles(pqv, m["built"], pqv.Searcher(self.index["built"], corpus), n_rows=c.n0)
            self.old_modes = {n: mc.resolve(oracle, m["built"], sp) for n, sp in mc.modes(name).items() if sp["metric"] != "cos"}
            self.old_before = {n: run(self.old, sp) for n, sp in self.old_modes.items()}
            self.old_mask_bytes = {n: h.to_bytes() for n, h in self.old.masks.items()}

        corpus.append(X[c.n0:c.n1])
        self.index["appended"] = self.index["built"].append(corpus)
        self._check_lists("appended")
        # (an appended index covers exactly the corpus' rows: its searchers are made now, the second one for relation 1)
        searcher = {}
        if searchers:
            searcher["appended"] = pqv.Searcher(self.index["appended"], corpus)
            under = pqv.Searcher(self.index["appended"], corpus)
        self.index["removed"] = self.index["appended"].remove(flags=c.flags)
        self._check_lists("removed")
        if searchers:
            searcher["removed"] = pqv.Searcher(self.index["removed"], corpus)
        corpus.append(X[c.n1:])
        grown = self.index["removed"].append(corpus)
        assert grown.to_bytes() == remove_ref.blob(oracle, c.dim, c.C, c.grown)
        self.index["chained"] = grown.remove(c.gone)
        self._check_lists("chained")
        if searchers:
            searcher["chained"] = pqv.Searcher(self.index["chained"], corpus)
        self.dense, self.index["compacted"], old_row = self.index["chained"].compact(corpus)
        assert np.array_equal(old_row, c.old_row)
        self._check_lists("compacted")
        self.keep = np.ones(c.n2, bool)                  # row_mask(~flags): what the remove left, and every later row
        self.keep[:c.n1] = ~c.flags
        if searchers:
            searcher["compacted"] = pqv.Searcher(self.index["compacted"], self.dense)
            self.h = {s: Handles(pqv, m[s], searcher[s]) for s in mc.MUTATED}
            self.under = Handles(pqv, m["appended"], under, keep=self.keep)
        self._memo = {}
        self.flags = {"row_order": _ffi.PQV_LAYOUT_ROW_ORDER, "prepare_cosine": _ffi.PQV_LAYOUT_IVF_ORDERED | _ffi.PQV_PREPARE_COSINE,
                      "release_row_order": _ffi.PQV_LAYOUT_IVF_ORDERED | _ffi.PQV_RELEASE_ROW_ORDER}

    def close(self):
        for h in list(self.h.values()) + [x for x in (self.old, self.under) if x is not None]:
            h.close()
        for ix in self.index.values():
            ix.close()
        self.dense.close()
        self.corpus.close()

    def _check_lists(self, state):
        from pq_vector_amd import _ffi
        c, m = self.case, self.case.models[state]
        assert np.array_equal(self.index[state].centroids.view(np.uint32), c.C.view(np.uint32)), state
        assert self.index[state].to_bytes() == remove_ref.blob(self.oracle, c.dim, c.C, m.lists), f"the lists of {state} are not the model's"
        assert self.index[state].row_bound == m.bound and self.index[state].n_rows == sum(len(l) for l in m.lists)
        assert _ffi.lib().pqv_index_row_bound(self.index[state]._h) == m.bound          # (the carried bound, not the largest id left + 1)

    def modes(self, state, group=None):
        key = (state, group)
        if key not in self._memo:
            self._memo[key] = {n: mc.resolve(self.oracle, self.case.models[state], sp) for n, sp in mc.modes(self.name).items()
                               if group is None or group_of(sp) == group}
        return self._memo[key]

    def expect(self, state, name):
        key = ("expect", state, name)
        if key not in self._memo:
            self._memo[key] = mc.expect(self.oracle, self.case.models[state], self.modes(state)[name])
        return self._memo[key]

    def got(self, state, name):
        """the library's answer on the state's main searcher, computed once (the relations compare it again)"""
        key = ("got", state, name)
        if key not in self._memo:
            self._memo[key] = run(self.h[state], self.modes(state)[name])
        return self._memo[key]


_ZOOS = {}


@pytest.fixture(scope="module")
def zoo(pqv, oracle):
    def get(name):
        if name not in _ZOOS:
            _ZOOS[name] = Zoo(pqv, oracle, name)
        return _ZOOS[name]
    yield get
    for z in _ZOOS.values():
        z.close()
    _ZOOS.clear()


def _route(z, state, metric="l2", nq=32):
    plan = z.h[state].s.describe(nq, mc.K, mc.NPROBE, METRIC[metric])
    if z.name in ("screened", "ties", "int8_256") and metric != "dot":          # mean list above plan_topk's 192-row rule in every state
        assert "wide_filter_kernel" in plan and ("int8 screen operands" in plan) == (z.name == "int8_256"), plan
    elif metric == "dot":
        assert "dot_stream_kernel" in plan, plan
    else:                                       # dim 30: the scalar exact kernels; dim 72: padded storage, short lists
        assert "wide_filter_kernel" not in plan and "tile_filter_kernel" not in plan, plan
    return plan


# ---- every mode against the numpy references -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", mc.MUTATED)
@pytest.mark.parametrize("name,group", CASE_GROUPS)
def test_mode_equals_the_references(zoo, name, state, group):
    z = zoo(name)
    _route(z, state)
    modes = z.modes(state, group)
    assert modes
    for mode, sp in modes.items():
        if sp["metric"] != "l2":
            _route(z, state, sp["metric"])
        mc.same(z.got(state, mode), z.expect(state, mode), what=f"{name} {state} {mode}")


@pytest.mark.parametrize("state", mc.MUTATED)
def test_ties_replay_the_heap(zoo, state):
    z = zoo("ties")
    s = z.h[state].s
    before = s.counters()["exact_replays"]
    sp = z.modes(state)["topk"]
    mc.same(run(z.h[state], sp), z.expect(state, "topk"), what=f"ties {state} topk")          # (the oracle's heap order)
    assert s.counters()["exact_replays"] > before


@pytest.mark.parametrize("state", mc.MUTATED)
@pytest.mark.parametrize("name", mc.CASES)
def test_an_emptied_list_is_probed_and_stepped_over(zoo, name, state):
    z = zoo(name)
    h, c = z.h[state], z.case
    sp = mc.spec("topk_device", nprobe=1)
    got = run(h, sp)
    mc.same(got, mc.expect(z.oracle, h.model, sp), what=f"{name} {state} nprobe 1")
    assert (state == "appended") == bool(got["nf"][0]) and (state == "appended") == bool(got["nc"][0])
    assert int(h.s.probe(c.Q[0], 1)[0]) == c.emptied


# ---- row masks keep the caller's bytes --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", mc.MUTATED)
@pytest.mark.parametrize("name", mc.CASES)
def test_row_masks_keep_the_callers_bytes_and_count_list_rows(zoo, pqv, name, state):
    z = zoo(name)
    h = z.h[state]
    inside = h.model.in_lists()
    for mask_name, mask in h.masks.items():
        a = h.mask_bytes[mask_name]
        assert mask.rows == h.n == len(a)
        assert np.array_equal(mask.to_bytes(), a.astype(np.uint8)), mask_name          # removed rows and rows past the bound included
        assert mask.count == int((a & inside).sum()), mask_name
    # a predicate over an attached column (int64 with NULLs): the mask the same bytes make
    pred = h.s.row_mask(pqv.col("ts") >= PRED_TS)
    ts, valid = h.model.cols["ts"]
    want = valid & (ts >= PRED_TS)
    assert np.array_equal(pred.to_bytes(), want.astype(np.uint8)) and pred.count == int((want & inside).sum())
    assert 0 < pred.count < int(inside.sum())
    by_bytes = h.s.row_mask(want)
    specs = [mc.spec("topk", mask=want), mc.spec("topk_device", mask=want, nprobe=z.case.nprobe_f)]
    if "range_masked" in z.modes(state):          # (int8_256 has no range modes)
        specs.append(dict(z.modes(state)["range_masked"], mask=want))
    for sp in specs:
        got = run(h, sp, mask=pred)
        mc.same(got, mc.expect(z.oracle, h.model, sp), what=f"{name} {state} predicate mask {sp['call']}")
        mc.same(run(h, sp, mask=by_bytes), got, what=f"{name} {state} predicate mask against its bytes")
    pred.close()
    by_bytes.close()


# ---- layouts and creation flags -----------------------------------------------------------------------------------------------------------
LAYOUT_MODES = ["topk", "topk_device", "topk_cosine", "topk_device_cosine", "topk_masked", "distinct", "keyed_eq", "range", "expand_masked",
                "depth_ratio", "depth_given_device", "depth_ratio_device_cosine"]


@pytest.mark.parametrize("layout", ["row_order", "prepare_cosine", "release_row_order"])
@pytest.mark.parametrize("state", mc.MUTATED)
@pytest.mark.parametrize("name", mc.CASES)
def test_layouts_and_creation_flags(zoo, pqv, name, state, layout):
    """PQV_LAYOUT_ROW_ORDER, PQV_PREPARE_COSINE, and PQV_RELEASE_ROW_ORDER on an uploaded copy with a cosine call first: on `removed` and
    `chained`, whose corpus holds rows of no list, that call builds the cosine layout with the row-order copy gone."""
    z = zoo(name)
    c, model = z.case, z.case.models[state]
    if state == "compacted":
        corpus, n = (pqv.Corpus.upload(model.X) if layout == "release_row_order" else z.dense), model.n
    elif state == "appended":          # (an appended index covers exactly its corpus' rows: a corpus of the n1 rows it was made on)
        corpus, n = pqv.Corpus.upload(c.X[:c.n1]), c.n1
    else:
        corpus, n = (pqv.Corpus.upload(c.X) if layout == "release_row_order" else z.corpus), c.n2
    h = Handles(pqv, model, pqv.Searcher(z.index[state], corpus, z.flags[layout]), n_rows=n)
    try:
        have = [m for m in LAYOUT_MODES if m in z.modes(state)]
        first = [m for m in ("topk_cosine", "topk_device_cosine") if m in have][:1] if layout == "release_row_order" else []
        assert len(have) >= 6 and (first or layout != "release_row_order")
        for mode in first + have:
            mc.same(run(h, z.modes(state)[mode]), z.expect(state, mode), what=f"{name} {state} {layout} {mode}")
    finally:
        h.close()


def _options():
    """the searcher options tests/test_gpu_table.py::test_table_answers_under_every_searcher_option iterates, read from that test"""
    import test_gpu_table
    marks = [m for m in test_gpu_table.test_table_answers_under_every_searcher_option.pytestmark if m.name == "parametrize"]
    assert len(marks) == 1 and marks[0].args[0] == "option,value", marks
    return [tuple(v) for v in marks[0].args[1]]


@pytest.mark.parametrize("option,value", _options())
def test_removed_answers_under_every_searcher_option(zoo, pqv, option, value):
    from pq_vector_amd import _ffi
    z = zoo("screened")
    model = z.case.models["removed"]
    s = pqv.Searcher(z.index["removed"], z.corpus, _ffi.PQV_LAYOUT_ROW_ORDER if option == "layout" else _ffi.PQV_LAYOUT_IVF_ORDERED)
    if option != "layout":
        s.set_option(option, value)
    h = Handles(pqv, model, s, masks=("dense",))
    try:
        for mode in ("topk", "topk_device", "topk_160", "topk_masked", "topk_device_masked", "topk_masked_160", "depth_given_device", "depth_ratio",
                     "depth_ratio_160"):
            mc.same(run(h, z.modes("removed")[mode]), z.expect("removed", mode), what=f"{option}={value} {mode}")
    finally:
        h.close()


# ---- relation 1: removed == appended under row_mask(~flags) ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,group", [(n, g) for n, g in CASE_GROUPS if g != "depth"])
def test_removed_equals_appended_under_the_keep_mask(zoo, name, group):
    """... n_candidates excepted; a filter on the removed side is the same filter combined with the mask on the old side.  With
    max_candidates the two differ by contract (the cap counts candidate positions, and the removed rows hold positions of the old
    lists only); so do pqv_topk's heap order and the masked call's (d2, position) order where distances tie.  The `depth` group has
    no part in this relation: pqv_topk_depth takes no mask, and every call on the old side is made under the keep mask."""
    z = zoo(name)
    assert np.array_equal(z.under.masks[None].to_bytes(), z.keep.astype(np.uint8))
    compared = 0
    for mode, sp in z.modes("removed", group).items():
        if sp["maxc"] or (name == "ties" and heap_order(sp)):
            continue
        mc.same(run(z.under, sp), z.got("removed", mode), skip=("nc",), what=f"{name} {mode}")
        compared += 1
    assert compared


# ---- relation 2: compacted == chained through old_row ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,group", CASE_GROUPS)
def test_compacted_equals_chained_through_old_row(zoo, name, group):
    z = zoo(name)
    old_row = z.case.old_row
    for mode in z.modes("compacted", group):
        new, old = dict(z.got("compacted", mode)), z.got("chained", mode)
        found = new["rows"] != mc.EMPTY
        new["rows"] = np.where(found, old_row[np.where(found, new["rows"], 0)], mc.EMPTY).astype(np.uint32)
        mc.same(new, old, what=f"{name} {mode}")          # ids, doc ids, distances, n_found, n_candidates, nprobe_used, lims


# ---- relation 3: old handles stay what they were -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.CASES)
def test_old_handles_answer_as_before_the_corpus_grew(zoo, pqv, name):
    z = zoo(name)
    c, old, model = z.case, z.old, z.case.models["built"]
    assert z.corpus.rows == c.n2 and old.n == c.n0
    for mode, sp in z.old_modes.items():          # the searcher, its masks and its keys, all made at n0 rows
        now = run(old, sp)
        mc.same(now, z.old_before[mode], what=f"{name} {mode} after the growth")
        mc.same(now, mc.expect(z.oracle, model, sp), what=f"{name} {mode} on built")
    for mask_name, mask in old.masks.items():
        assert mask.rows == c.n0 and np.array_equal(mask.to_bytes(), z.old_mask_bytes[mask_name])
    # a first cosine call after the growth: the reference over `built`
    for mode in [m for m in ("topk_cosine", "topk_device_cosine") if m in mc.modes(name)]:
        sp = mc.resolve(z.oracle, model, mc.modes(name)[mode])
        mc.same(run(old, sp), mc.expect(z.oracle, model, sp), what=f"{name} {mode} on built, first cosine call after the growth")
    # a mask or row keys made NOW take the corpus' current row count; the old length is refused
    with pytest.raises(pqv.PqvError, match=f"row mask has {c.n0} rows, the corpus has {c.n2}"):
        old.s.row_mask(model.masks["dense"][:c.n0])
    short = pqv.Column.upload(model.cols["tenant"][0][:c.n0])
    with pytest.raises(pqv.PqvError, match=f"column has {c.n0} rows, the corpus has {c.n2}"):
        old.s.row_keys(short)
    short.close()
    late = Handles(pqv, model, old.s, n_rows=c.n2)
    try:
        for mask_name, mask in late.masks.items():
            assert mask.rows == c.n2 and np.array_equal(mask.to_bytes(), late.mask_bytes[mask_name].astype(np.uint8))
            assert mask.count == int((late.mask_bytes[mask_name] & model.in_lists()).sum())
        for mode, sp in z.old_modes.items():
            if sp["mask"] or sp["filt"] or group_of(sp) == "distinct":
                mc.same(run(late, sp), z.old_before[mode], what=f"{name} {mode} with handles made after the growth")
    finally:
        for h in list(late.masks.values()) + list(late.keys.values()):
            h.close()


# ---- removed rows never reach an answer --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["ivf_ordered", "row_order"])
@pytest.mark.parametrize("name", ["screened", "exact30"])
def test_removed_rows_are_never_read(zoo, pqv, name, layout):
    """every removed row overwritten with NaN, +-inf and 1e30: every mode's outputs on `removed` are what they are on the clean
    corpus (the route may differ: norms and the finiteness scan cover every corpus row)"""
    from pq_vector_amd import _ffi
    z = zoo(name)
    c, model = z.case, z.case.models["removed"]
    X = c.X.copy()
    gone = np.nonzero(~model.in_lists()[:c.n1])[0]
    poison = np.array([np.nan, np.inf, -np.inf, 1e30], np.float32)
    X[gone] = poison[(np.arange(len(gone))[:, None] + np.arange(c.dim)[None, :]) % 4]
    flags = _ffi.PQV_LAYOUT_ROW_ORDER if layout == "row_order" else _ffi.PQV_LAYOUT_IVF_ORDERED
    h = Handles(pqv, model, pqv.Searcher(z.index["removed"], pqv.Corpus.upload(X), flags))
    try:
        for mode, sp in z.modes("removed").items():
            mc.same(run(h, sp), z.expect("removed", mode), what=f"{name} {layout} {mode} over poisoned removed rows")
    finally:
        h.close()
