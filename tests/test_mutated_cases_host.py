"""The premises of tests/mutated_cases.py, checked on the CPU with the numpy references: the zoo of mutated indexes is not vacuous,
so no GPU test of tests/test_gpu_mutated_search.py needs a skip or an `if`.  A premise that a seed misses is met by another seed,
never by a weaker premise."""
import numpy as np
import pytest

import append_ref
import depth_ref
import distinct_expand_ref
import expand_ref
import mutated_cases as mc
from range_oracle import REF4, SEQ, l2_chain

EMPTY_STATES = ["removed", "chained", "compacted"]          # the states in which the emptied list is empty
FILTERED = {"mask": dict(mask="sparse"), "key equality": dict(filt="eq"), "key set": dict(filt="in"), "key range": dict(filt="range")}


@pytest.fixture(scope="module", params=mc.CASES + ["probe32"])
def case(request, oracle):
    return mc.case(oracle, request.param)


def test_states_are_what_the_table_says(case):
    m = case.models
    n0, n1, n2 = case.n0, case.n1, case.n2
    count = lambda s: sum(len(l) for l in m[s].lists)          # noqa: E731
    assert count("built") == n0 and count("appended") == n1
    assert 0.55 * n1 < count("removed") < 0.68 * n1
    assert case.flags[n1 - 30:].all() and append_ref.row_bound(m["removed"].lists) < n1 == m["removed"].bound
    assert count("chained") < count("removed") + (n2 - n1) and m["chained"].bound == n2
    assert count("compacted") == count("chained") == len(case.old_row) == m["compacted"].n
    for s in EMPTY_STATES:
        assert len(m[s].lists[case.emptied]) == 0
    assert sorted(np.concatenate(m["compacted"].lists).tolist()) == list(range(len(case.old_row)))
    assert len(set(case.gone.tolist())) < len(case.gone) and (case.gone >= n2).any()          # duplicates, unindexed ids
    assert not (np.diff(case.gone[:500].astype(np.int64)) > 0).all()
    if case.name in ("screened", "ties"):          # plan_topk's 192-row rule: the mean list stays above it in every state
        assert all(count(s) / case.kc > 192 for s in mc.STATES)
    if case.name == "padded72":
        assert all(count(s) / case.kc < 192 for s in mc.STATES)
    doc, _ = m["compacted"].cols["doc"]
    assert (doc == m["chained"].cols["doc"][0][case.old_row]).all()


def test_queries_reach_the_emptied_list_and_a_removed_row(case, oracle):
    for s in EMPTY_STATES:
        model = case.models[s]
        oidx = model.oidx(oracle)
        first = np.stack([oidx.find_closest_centroids(q, mc.NPROBE) for q in case.Q])
        assert (first == case.emptied).any(axis=1).sum() >= 1
        assert int(oidx.find_closest_centroids(case.Q[0], 1)[0]) == case.emptied
        e = mc.expect(oracle, model, mc.spec("topk_device", nprobe=1))
        assert e["nf"][0] == 0 and e["nc"][0] == 0 and (e["rows"][0] == mc.EMPTY).all()
        assert (e["nf"][1:] > 0).any()
    hit = np.nonzero((case.X[:case.n1] == case.Q[1]).all(axis=1))[0]
    assert len(hit) == 1 and case.flags[hit[0]] and not case.models["removed"].in_lists()[hit[0]]
    assert case.models["appended"].in_lists()[hit[0]]


@pytest.mark.parametrize("state", mc.MUTATED)
@pytest.mark.parametrize("which", list(FILTERED))
def test_every_filter_has_queries_on_both_sides_of_k_and_at_three_depths(case, oracle, state, which):
    model = case.models[state]
    sp = mc.spec("topk", nprobe=case.nprobe_f, maxp=case.max_nprobe, **FILTERED[which])
    inside = mc.passing_in(oracle, model, sp, case.nprobe_f)
    assert (inside < mc.K).any() and (inside >= mc.K).any(), inside
    allow = mc.allowed_rows(model, sp, len(case.Q))
    used = expand_ref.used_for_batch(model.oidx(oracle), model.lists, allow, case.Q, mc.K, case.nprobe_f, case.max_nprobe)
    assert (used == case.nprobe_f).any() and ((used > case.nprobe_f) & (used < case.max_nprobe)).any() and (used == case.max_nprobe).any(), used
    assert (mc.expect(oracle, model, sp)["used"] == used).all()


@pytest.mark.parametrize("state", mc.MUTATED)
def test_the_distinct_depths_differ_too(case, oracle, state):
    model = case.models[state]
    group, gvalid = model.cols["doc"]
    for kw in (dict(mask="sparse"), dict(filt="eq")):
        sp = mc.spec("distinct", nprobe=case.nprobe_f, maxp=case.max_nprobe, **kw)
        allow = mc.allowed_rows(model, sp, len(case.Q))
        used = distinct_expand_ref.used_for_batch(model.oidx(oracle), model.lists, group, gvalid, allow, case.Q, mc.K, case.nprobe_f,
                                                  case.max_nprobe)
        assert (used == case.nprobe_f).any() and ((used > case.nprobe_f) & (used < case.max_nprobe)).any() and (used == case.max_nprobe).any(), used
        assert (mc.expect(oracle, model, sp)["used"] == used).all()


def depth_premises(oracle, case, states):
    """The per-query depth modes of one case are not vacuous, on the REFERENCE's depths alone (tests/depth_ref.py over the oracle):
    the ratio draw has at least three distinct depths, the floor p0 among them and, for L2, the ceiling P; query 0 -- the emptied
    list's centroid, d2_0 == 0 -- counts one rank and walks p0 lists, so that in the states where that list is empty it gets
    nothing (p0 == 1) or its second list alone (p0 == 2)."""
    p0, P = case.nprobe_f, case.max_nprobe
    modes = mc.modes(case.name)
    assert 1 <= p0 <= 2 and p0 + 1 < P <= case.kc
    for state in states:
        model = case.models[state]
        for name, metric in (("depth_ratio_device", "l2"), ("depth_ratio_device_cosine", "cos")):
            sp = mc.resolve(oracle, model, modes[name])
            assert sp["metric"] == metric and (sp["nprobe"], sp["maxp"]) == (p0, P) and isinstance(sp["ratio"], float) and sp["ratio"] > 1
            used = mc.depth_used(oracle, model, sp)
            depths = set(used.tolist())
            print(f"{case.name} {state} {metric}: p0 {p0} P {P} ratio {sp['ratio']:.4f} at p0 {int((used == p0).sum())} at P {int((used == P).sum())} "
                  f"distinct {len(depths)}")
            assert len(depths) >= 3 and p0 in depths and (metric != "l2" or P in depths), (name, state, used)
            for other in [n for n, o in modes.items() if o["ratio"] is not None and o["metric"] == metric and not o["q160"]]:
                assert mc.resolve(oracle, model, modes[other])["ratio"] == sp["ratio"], other          # (one draw per metric)
        # query 0 under L2
        sp = mc.resolve(oracle, model, modes["depth_ratio_device"])
        oidx = model.oidx(oracle)
        d2 = depth_ref.probe_d2(oracle, oidx, case.Q[0], P)
        assert d2[0] == 0 and depth_ref.ratio_count(d2, sp["ratio"]) == 1 and mc.depth_used(oracle, model, sp)[0] == p0
        assert int(depth_ref.probe_order(oidx, case.Q[0], P)[0]) == case.emptied
        given = modes["depth_given_device"]
        assert given["depths"][0] == 0 and mc.depth_used(oracle, model, given)[0] == p0
        assert {p0, (p0 + P) // 2, P} <= set(mc.depth_used(oracle, model, given).tolist()) and{0, P + 1, 2 ** 32 - 1} <= set(given["depths"].tolist())
        if state in EMPTY_STATES:
            second = len(model.lists[int(depth_ref.probe_order(oidx, case.Q[0], 2)[1])])
            for name in ("depth_ratio", "depth_ratio_device", "depth_given", "depth_given_device"):
                e = mc.expect(oracle, model, mc.resolve(oracle, model, modes[name]))
                assert e["used"][0] == p0
                if p0 == 1:
                    assert e["nf"][0] == 0 and e["nc"][0] == 0 and (e["rows"][0] == mc.EMPTY).all(), (name, state)
                else:
                    assert e["nc"][0] == second > 0 and e["nf"][0] == min(mc.K, second), (name, state)
                assert (e["nf"][1:] > 0).any() and len(set(e["nc"].tolist())) > 3


def test_the_depth_draws_are_not_vacuous(case, oracle):
    depth_premises(oracle, case, mc.STATES)
    # the depths depend on the centroids alone: one draw for all five states
    for name in ("depth_ratio", "depth_ratio_cosine", "depth_given_device"):
        if name in mc.modes(case.name):
            used = [mc.depth_used(oracle, case.models[s], mc.resolve(oracle, case.models[s], mc.modes(case.name)[name])) for s in mc.STATES]
            assert all((u == used[0]).all() for u in used)


def test_the_depth_modes(oracle):
    """which depth modes a case has: all of them on int8_256, the host cosine form off the integer cases, the 160-query batch on
    `screened` alone; k = 1000 is above one list's rows, so a query at depth 1 gets every candidate"""
    names = {"depth_given", "depth_given_device", "depth_ratio", "depth_ratio_device", "depth_ratio_k1", "depth_given_device_k1000",
             "depth_given_device_nq1", "depth_ratio_cosine", "depth_ratio_device_cosine"}
    for case_name in mc.CASES + ["probe32", "far768", "far768i"]:
        have = {n for n, sp in mc.modes(case_name).items() if mc.is_depth(sp)}
        want = names - ({"depth_ratio_cosine"} if mc.SHAPES[case_name]["integer"] else set())
        if case_name == "screened":
            want |= {"depth_ratio_160", "depth_given_device_160"}
        assert have == want, case_name
        for n in have:
            sp = mc.modes(case_name)[n]
            assert sp["sqrt"] == (sp["call"] == "topk" and sp["metric"] == "l2") and sp["maxp"] > sp["nprobe"], n
    case = mc.case(oracle, "screened")
    for state in mc.MUTATED:
        model = case.models[state]
        e = mc.expect(oracle, model, mc.modes("screened")["depth_given_device_k1000"])
        assert e["used"].tolist() == [1, 2] * 16
        short = (e["used"] == 1) & (e["nc"] < 1000)
        assert short.sum() >= 8 and (e["nf"][short] == e["nc"][short]).all() and (e["nc"][e["used"] == 2] > 1000).any(), (e["used"], e["nc"])


def test_masks_allow_removed_rows_and_keys_match_them(case):
    m = case.models
    for s in ("removed", "chained"):
        out = ~m[s].in_lists()
        assert out[:m[s].bound].sum() > 100
        for name in ("dense", "sparse"):
            assert (m[s].masks[name] & out).any()
    assert m["removed"].masks["dense"][case.n1:].any()          # ... and rows past the index' bound
    tenant, _ = m["removed"].cols["tenant"]
    gone = ~m["removed"].in_lists()[:case.n1]
    assert ((tenant[:case.n1] == case.qkeys[1]) & gone).any()
    ts, valid = m["removed"].cols["ts"]
    assert ts.dtype == np.int64 and ts.min() > 2 ** 32 and 0 < (~valid).sum() < len(valid) and tenant.dtype == np.int32


@pytest.mark.parametrize("state", mc.MUTATED)
@pytest.mark.parametrize("name,metric", [(n, m) for n in mc.CASES for m, mode in (("l2", "range"), ("cos", "range_cosine"), ("dot", "dot_range"))
                                         if mode in mc.modes(n)])
def test_the_range_radius_cuts_every_query(oracle, state, name, metric):
    case = mc.case(oracle, name)
    model = case.models[state]
    sp = mc.resolve(oracle, model, mc.spec("range", metric=metric))
    e = mc.expect(oracle, model, sp)
    assert ((e["nw"] > 0) & (e["nw"] < e["nc"])).all(), (e["nw"], e["nc"])
    capped = mc.expect(oracle, model, dict(sp, maxc=mc.CAP, maxr=5))
    assert (np.diff(capped["lims"].astype(np.int64)) <= 5).all() and (capped["nw"] <= e["nw"]).all() and (capped["nw"] < e["nw"]).any()


def test_ties_hold_ties_at_the_kth_place(oracle):
    case = mc.case(oracle, "ties")
    for state in mc.MUTATED:
        model = case.models[state]
        tied = 0
        for q in case.Q:
            cand = model.oidx(oracle).candidate_rows(q, mc.NPROBE).astype(np.int64)
            d2 = np.sort(l2_chain(model.X[cand], q, REF4))
            assert (l2_chain(model.X[cand], q, SEQ).view(np.uint32) == l2_chain(model.X[cand], q, REF4).view(np.uint32)).all()
            tied += bool(d2[mc.K - 1] == d2[mc.K])
        assert tied >= len(case.Q) // 4, tied


def test_caps_fall_below_at_and_above_the_candidates(case, oracle):
    for state in mc.MUTATED:
        model = case.models[state]
        nc = mc.expect(oracle, model, mc.spec("topk_device"))["nc"]
        at = mc.resolve(oracle, model, mc.spec("topk", maxc=None))["maxc"]
        assert at == nc[0] and (nc > mc.CAP).all() and (nc < (1 << 20)).all()
        one = mc.expect(oracle, model, mc.spec("topk_device", k=1024, nprobe=1))
        short = one["nf"] < 1024          # k above the candidates of one list: the answer is every candidate
        assert short.sum() >= len(short) // 2 and (one["nf"][short] == one["nc"][short]).all()
