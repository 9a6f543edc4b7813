"""The premises of tests/far_rows_cases.py, checked on the CPU with the numpy references: the relocation puts listed rows on both sides
of every offset at which 32-bit address arithmetic breaks, in every state tests/test_gpu_far_rows.py searches or mutates, and the
answers it expects come from those rows.  A premise that a seed misses is met by another seed, never by a weaker premise."""
import numpy as np
import pytest

import far_rows_cases as frc
import mutated_cases as mc
from range_oracle import REF4, l2_chain

NAMES = ["far768", "far768i"]
STATES = ["appended", "removed", "chained"]
NEAR = 8


@pytest.fixture(scope="module", params=NAMES)
def far(request, oracle):
    return frc.far_case(oracle, request.param)


def test_the_break_rows_and_the_map(far):
    c, R = far.case, far.R
    assert far.breaks == frc.break_rows(768) == [699050, 1398101, 2796202, 5592405]
    for r, x in zip(far.breaks, (1 << 31, 1 << 32)):                      # bytes
        assert r * 768 * 4 < x < (r + 1) * 768 * 4 - 4
    for r, x in zip(far.breaks[2:], (1 << 31, 1 << 32)):                  # elements
        assert r * 768 < x < (r + 1) * 768 - 1
    assert len(R) == c.n2 and (np.diff(R) > 0).all() and R[0] == 0
    # the runs: consecutive rows, each break row in the middle of its own
    runs = [(768, 1536), (1536, 2304), (2304, 3072), (c.n0, c.n1)]
    for (lo, hi), b in zip(runs, far.breaks):
        assert (np.diff(R[lo:hi]) == 1).all() and R[lo] == b - (hi - lo) // 2 and R[lo] < b < R[hi - 1]
    assert (np.diff(R[:768]) == 1).all() and (np.diff(R[c.n1:]) == 1).all() and R[c.n1] == R[c.n1 - 1] + 1 + frc.GAP
    assert far.n_far == R[-1] + 1 == 5594429 and 16.0 < far.n_far * 768 * 4 / 2 ** 30 < 16.01
    assert far.n_far * 768 > 1 << 32 and far.n_far < 1 << 32
    # what the library's append is given: the appended ranges are contiguous
    assert far.bound(c.n1) == R[c.n0] + (c.n1 - c.n0) and far.bound(c.n2) == far.n_far == R[c.n1] + (c.n2 - c.n1)
    assert R[c.n0] >= far.bound(c.n0) and R[c.n1] >= far.bound(c.n1)
    ids = np.concatenate([c.gone, [0, c.n2 - 1]]).astype(np.uint32)
    moved = far.rows(ids)
    assert moved[-3] == mc.EMPTY and moved[-4] == c.n2 + 5 and moved[-1] == far.n_far - 1 and (moved[:-4] == R[c.gone[:-2].astype(np.int64)]).all()


def test_the_shapes(far):
    c = far.case
    sh = mc.SHAPES[far.name]
    assert far.name not in mc.CASES and c.integer == sh["integer"] == (far.name == "far768i")
    assert (c.dim, c.kc, c.n0, c.n1, c.n2) == (768, 8, 3072, 4096, 4608)
    # the images-only layout: rows of a multiple of 64 dims, a mean list of at least 192 rows -- in every state
    for s in mc.STATES:
        assert sum(len(l) for l in c.models[s].lists) // c.kc >= 192, s
    specs = mc.modes(far.name)
    groups = {g: [n for n, sp in specs.items() if _group(sp) == g] for g in ("plain", "masks", "metrics", "keys", "expand", "distinct", "range", "depth")}
    assert set(groups) == set(_groups())
    assert all(groups.values())
    if far.name == "far768":
        assert {"dot", "dot_device", "dot_range", "dot_masked", "dot_range_masked"} <= set(specs)
        assert set(specs) - {"dot", "dot_device", "dot_range", "dot_masked", "dot_range_masked"} == set(mc.modes("probe32"))


def _group(sp):
    import mode_calls
    return mode_calls.group_of(sp)


def _groups():
    import mode_calls
    return mode_calls.GROUPS


def test_the_depth_draws_are_not_vacuous(far, oracle):
    """the premises of the per-query depth modes (tests/test_mutated_cases_host.py), on the states the far tests search"""
    from test_mutated_cases_host import depth_premises
    depth_premises(oracle, far.case, mc.STATES)
    dense = far.case.models["chained"]
    for name in ("depth_ratio_device", "depth_given_device"):
        e = mc.expect(oracle, dense, mc.resolve(oracle, dense, mc.modes(far.name)[name]))
        moved = far.relocate(e)
        found = e["rows"] != mc.EMPTY
        assert (moved["rows"][found] == far.R[e["rows"][found].astype(np.int64)]).all() and (moved["rows"][~found] == mc.EMPTY).all()
        assert (moved["used"] == e["used"]).all() and (moved["rows"][found] > far.breaks[-1]).any()


@pytest.mark.parametrize("state", STATES)
def test_listed_rows_lie_on_both_sides_of_every_break(far, state):
    """... and close to it: the break row itself where the state still lists it, else listed rows within NEAR rows on either side"""
    m = far.model(state)
    inside = m.in_lists()
    assert inside.sum() == sum(len(l) for l in far.case.models[state].lists) and m.n == far.n_far
    lo_of = {b: int(far.R[lo]) for b, lo in zip(far.breaks, (768, 1536, 2304, far.case.n0))}
    hi_of = {b: int(far.R[hi - 1]) for b, hi in zip(far.breaks, (1536, 2304, 3072, far.case.n1))}
    listed = []
    for b in far.breaks:
        below, above = np.nonzero(inside[lo_of[b]:b])[0], np.nonzero(inside[b + 1:hi_of[b] + 1])[0]
        assert len(below) > 100 and len(above) > 100, (state, b)
        listed.append(bool(inside[b]))
        if not inside[b]:
            assert (b - lo_of[b]) - below[-1] <= NEAR and above[0] + 1 <= NEAR, (state, b)
    if state == "appended":
        assert all(listed)              # (nothing removed yet: every break row is a listed row)
    print(f"{far.name} {state}: break rows listed: {dict(zip(far.breaks, listed))}")


def test_filler_rows_would_change_an_answer(far):
    c, m = far.case, far.model("chained")
    filler = np.ones(far.n_far, bool)
    filler[far.R] = False
    assert filler.sum() == far.n_far - c.n2 and not (filler & m.in_lists()).any()
    assert m.masks["dense"][filler].all() and m.masks["sparse"][filler].all()
    tenant, _ = m.cols["tenant"]
    ts, valid = m.cols["ts"]
    lo, hi = c.filters["range"][2]
    assert (tenant[filler] == c.qkeys[0]).all() and valid[filler].all() and (m.cols["doc"][0][filler] == 0).all()
    assert ((ts[filler] >= lo[0]) & (ts[filler] <= hi[0])).all()
    for name, (v, ok) in m.cols.items():
        dv, dok = c.models["chained"].cols[name]
        assert v.dtype == dv.dtype and (v[far.R] == dv).all() and (ok is None or (ok[far.R] == dok).all())
    for name, a in m.masks.items():
        assert (a[far.R] == c.models["chained"].masks[name]).all()
    if not c.integer:          # uniform data: a row of 0.5s is nearer to every query than any real row
        d_fill = ((c.Q.astype(np.float64) - 0.5) ** 2).sum(axis=1)
        d_real = ((c.Q[:, None, :].astype(np.float64) - c.X[None, ::37, :]) ** 2).sum(axis=2).min(axis=1)
        near = np.arange(len(c.Q)) % 4 != 3          # (the queries beside a corpus row have that row nearer still)
        assert (d_fill[~near] < d_real[~near]).all()


@pytest.mark.parametrize("wrap", [1 << 30, 1 << 32], ids=["u32_bytes", "u32_elements"])
def test_a_wrapped_offset_changes_every_distance_above_its_break(oracle, wrap):
    """what the GPU tests rely on: a kernel that formed a row's byte offset, or row * dim, in 32 unsigned bits would read, for every
    listed row above that break, other data than the row's -- parts of two rows, real or filler -- and compute another distance to
    every query.  (The signed forms leave the buffer instead.)"""
    far = frc.far_case(oracle, "far768")
    c = far.case
    listed = np.nonzero(c.models["chained"].in_lists())[0]
    above = listed[far.R[listed] * c.dim >= wrap]
    assert len(above) > 300 and len(above) < len(listed)
    for i in above[:: max(1, len(above) // 60)]:
        got = far.read((int(far.R[i]) * c.dim) % wrap, 0.5)
        assert (far.read(int(far.R[i]) * c.dim, 0.5) == c.X[i]).all() and (got != c.X[i]).any()
        for q in c.Q[:8]:
            d_true, d_got = l2_chain(c.X[i][None, :], q, REF4), l2_chain(got[None, :], q, REF4)
            assert d_true.view(np.uint32)[0] != d_got.view(np.uint32)[0]


def test_the_integer_shape_ties_at_the_kth_place(oracle):
    """... for several queries, so that pqv_topk replays the heap over rows it fetches from the far corpus"""
    c = frc.far_case(oracle, "far768i").case
    model = c.models["chained"]
    tied = 0
    for q in c.Q:
        cand = model.oidx(oracle).candidate_rows(q, mc.NPROBE).astype(np.int64)
        d2 = np.sort(l2_chain(model.X[cand], q, REF4))
        tied += bool(d2[mc.K - 1] == d2[mc.K])
    assert tied >= 4, tied


def test_the_range_radius_has_queries_of_every_kind(oracle):
    """768 uniform dims: no radius has hits and cuts for every query (mutated_cases.pick_radius); the one taken leaves some queries
    nothing, some a part of their candidates, and the unfiltered L2 call one query every candidate"""
    far = frc.far_case(oracle, "far768")
    dense = far.case.models["chained"]
    for name in ("range", "range_masked", "range_keyed_in", "dot_range"):
        e = mc.expect(oracle, dense, mc.resolve(oracle, dense, mc.modes("far768")[name]))
        some = int(((e["nw"] > 0) & (e["nw"] < e["nc"])).sum())
        assert some >= 8 and (name == "dot_range" or (e["nw"] == 0).any()) and e["lims"][-1] > 20, (name, e["nw"], e["nc"])
        assert name != "range" or ((e["nw"] == e["nc"]) & (e["nc"] > 0)).any()


def test_the_expected_rows_reach_above_every_break(far, oracle):
    """over the batch, the answers of the plain, masked, keyed, distinct and dot top-k on `chained` hold rows above each of the four
    breaks (and below the first): a change of seed cannot silently empty a band"""
    c, dense = far.case, far.case.models["chained"]
    names = ["topk", "topk_masked", "keyed_eq", "distinct"] + (["dot"] if far.name == "far768" else [])
    for name in names:
        sp = mc.resolve(oracle, dense, mc.modes(far.name)[name])
        e = far.relocate(mc.expect(oracle, dense, sp))
        rows = e["rows"][e["rows"] != mc.EMPTY].astype(np.int64)
        assert len(rows) > 0 and (rows < far.n_far).all() and dense.in_lists()[np.searchsorted(far.R, rows)].all()
        edges = [0] + far.breaks + [far.n_far]
        bands = [int(((rows > a) & (rows <= b)).sum()) for a, b in zip(edges[:-1], edges[1:])]
        assert all(n > 0 for n in bands[1:]) and (rows < far.breaks[0]).any(), (name, bands)
        print(f"{far.name} chained {name}: answer rows per band {bands}")
