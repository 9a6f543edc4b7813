"""Every search mode under the screened centroid probe (probe_screen_kernel + probe_resolve_kernel).  enqueue_probe sits
behind every entry point -- plain, capped, per-query depths (whose ratio rule reads the probe distances the merge hands out: MergeArgs::
probe_d2), masked, keyed (EQ / IN / RANGE), expanding, distinct, grouped, their device forms, range and cosine -- and each hands it another request (an expanding call ranks max_nprobe lists, cosine goes through the lazily made inner
searcher, which copies the options) and other scratch to zero on the way.

The shape `probe32` of tests/mutated_cases.py has 32 centroids and no depth above 8 = kc / 4, so the screen is eligible in every call
of mutated_cases.modes().  Two of its states are searched, `built` and `removed` (fewer list rows than corpus rows, one empty list),
each index made from the model's blob, by two searchers: probe_screen = 2 and = 0.  Every output of every call is the same on
both and equal to mutated_cases.expect() -- numpy over the oracle -- bit for bit, nprobe_used of the expanding calls included.
tests/test_mutated_cases_host.py holds the shape to the zoo's premises."""
import re

import pytest

import mutated_cases as mc
import remove_ref
from mode_calls import GROUPS, METRIC, Handles, group_of, run

pytestmark = pytest.mark.gpu

NAME = "probe32"
STATES = ["built", "removed"]
SCREENED = "probe_screen_kernel + probe_resolve_kernel"
BATCHED = 8          # pqv.h, "probe_rows": the batched probe -- the one the screen replaces -- runs from 8 queries on


def _handles(pqv, oracle, model, bound, option):
    c = model.case
    index = pqv.Index.from_bytes(remove_ref.blob(oracle, c.dim, c.C, model.lists))
    s = pqv.Searcher(index, pqv.Corpus.upload(c.X[:bound]))
    s.set_option("probe_screen", option)
    return Handles(pqv, model, s, n_rows=bound)


class Pair:
    """One state: the screened searcher, the exact one, and the resolved specs with their expectations."""

    def __init__(self, pqv, oracle, state):
        self.case = c = mc.case(oracle, NAME)
        self.model = c.models[state]
        self.bound = {"built": c.n0, "removed": c.n1}[state]
        assert self.model.bound == self.bound
        self.h2 = _handles(pqv, oracle, self.model, self.bound, 2)
        self.h0 = _handles(pqv, oracle, self.model, self.bound, 0)
        self.modes = {n: mc.resolve(oracle, self.model, sp) for n, sp in mc.modes(NAME).items()}
        self.oracle = oracle

    def close(self):
        self.h2.close()
        self.h0.close()


@pytest.fixture(scope="module")
def pairs(pqv, oracle):
    made = {}

    def get(state):
        if state not in made:
            made[state] = Pair(pqv, oracle, state)
        return made[state]
    yield get
    for p in made.values():
        p.close()


def test_the_shape_keeps_every_depth_eligible():
    sh = mc.SHAPES[NAME]
    specs = mc.modes(NAME)
    assert len(specs) == 78 and not any(sp["metric"] == "dot" for sp in specs.values())
    assert {sp["maxp"] or sp["nprobe"] for sp in specs.values()} == {1, 2, 4, 8} and sh["max_nprobe"] == 8 == sh["kc"] // 4
    assert {group_of(sp) for sp in specs.values()} == set(GROUPS)
    assert NAME not in mc.CASES


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("state", STATES)
def test_mode_under_the_screen(pairs, state, group):
    p = pairs(state)
    modes = {n: sp for n, sp in p.modes.items() if group_of(sp) == group}
    assert modes
    for mode, sp in modes.items():
        what = f"{NAME} {state} {mode}"
        got2, got0 = run(p.h2, sp), run(p.h0, sp)
        mc.same(got2, got0, what=what + ": screened against exact")
        mc.same(got2, mc.expect(p.oracle, p.model, sp), what=what)
        if sp["k"] >= 1024:          # (pqv_topk with k >= 1024 probes on the host, and describe() speaks of the device form)
            continue
        # the route, after the call (a first cosine call makes the inner searcher, which describe() then speaks of)
        nq, depth = len(p.case.queries(sp)), sp["maxp"] or sp["nprobe"]
        d2 = p.h2.s.describe(nq, sp["k"], depth, METRIC[sp["metric"]])
        d0 = p.h0.s.describe(nq, sp["k"], depth, METRIC[sp["metric"]])
        assert (SCREENED in d2) == (nq >= BATCHED), (what, d2)
        assert SCREENED not in d0, (what, d0)


def test_the_option_reaches_the_expanding_plan_and_the_cosine_searcher(pqv, oracle, monkeypatch, capfd):
    """PQV_PROBE_SCREEN_STATS=1: the counters a searcher prints when it is freed.  The expanding, distinct and cosine calls on ONE
    screened searcher: the L2 searcher counted the queries of every L2 call, and the cosine searcher -- made by the first cosine
    call, with the options copied -- prints a line of its own with the queries of the cosine calls."""
    monkeypatch.setenv("PQV_PROBE_SCREEN_STATS", "1")
    c = mc.case(oracle, NAME)
    model = c.models["removed"]
    capfd.readouterr()
    h = _handles(pqv, oracle, model, c.n1, 2)
    n_l2 = n_cos = 0
    for mode, sp in mc.modes(NAME).items():
        if not (sp["maxp"] or sp["metric"] == "cos" or group_of(sp) == "distinct"):
            continue
        sp = mc.resolve(oracle, model, sp)
        mc.same(run(h, sp), mc.expect(oracle, model, sp), what=f"{NAME} removed {mode}")
        if sp["metric"] == "cos":
            n_cos += len(c.queries(sp))
        else:
            n_l2 += len(c.queries(sp))
    assert n_cos >= 4 * 32 and n_l2 >= 20 * 32
    h.close()
    err = capfd.readouterr().err
    counted = sorted(int(m.group(1)) for m in re.finditer(r"screened probe: (\d+) queries, ", err))
    # every call probes its batch at least once (an expanding call that re-ranks may probe again): two searchers, two lines
    assert len(counted) == 2 and counted[0] >= min(n_cos, n_l2) and counted[1] >= max(n_cos, n_l2) and counted[0] > 0, err
