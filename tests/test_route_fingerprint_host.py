"""tools/route_fingerprint.py without a GPU: its call list names every request kind in both forms, and its comparison excludes exactly
the counters that differ between runs of one library."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fp():
    spec = importlib.util.spec_from_file_location("route_fingerprint", os.path.join(ROOT, "tools", "route_fingerprint.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_call_list_names_every_request_kind_in_both_forms(fp):
    names = [c["name"] for c in fp.cases()]
    assert len(names) == len(set(names))
    host = [n for n in names if n + "_device" in names]
    for kind in ("plain_k10", "plain_k100", "plain_k300", "dot", "cosine", "masked", "expand_mask", "expand_filter", "distinct", "grouped_m1",
                 "grouped_m3", "distinct_filtered", "grouped_filtered", "distinct_expand", "grouped_expand"):
        assert kind in host, kind
    for filt in ("eq", "range", "in"):
        for width in ("i32", "i64"):
            assert f"keyed_{filt}_{width}" in host and f"keyed_{filt}_{width}_mask" in host
    for route in ("table_cap", "tile_rerank", "tile_filter_f32", "padded", "q_global", "deferred", "range", "range_masked", "range_dot",
                  "range_host_probe", "wide_i8_one", "wide_i8_batch", "wide_f16_one", "wide_f16_batch", "wide_f32_one", "wide_f32_batch"):
        assert route in names, route
    for c in fp.cases():        # a route case says what the describe string must show; a request case must find rows (checked in the run)
        assert c["expect"] or c["name"].split("_device")[0] in host or c["kind"] == "range", c["name"]
        assert c["data"] in fp.DATASETS


def _run(fp, path, **over):
    rows = [{"call": "a", "sha256": "11", "describe": "stream", "counters": {"queries": 8, "screen_survivors": 1}},
            {"call": "b", "sha256": "22", "describe": "screen", "counters": {"queries": 700, "screen_survivors": 5000}}]
    for call, fields in over.items():
        for r in rows:
            if r["call"] == call:
                for k, v in fields.items():
                    (r["counters"] if k in r["counters"] else r).__setitem__(k, v)
    fp.write_results(str(path), rows)
    assert fp.load_results(str(path)) == {r["call"]: r for r in rows}
    return str(path)


def test_compare_excludes_only_what_the_same_library_varies_in(fp, tmp_path, capsys):
    parent = _run(fp, tmp_path / "p.json")
    again = _run(fp, tmp_path / "p2.json", b={"screen_survivors": 5003})
    new = _run(fp, tmp_path / "n.json", b={"screen_survivors": 4999})
    with pytest.raises(SystemExit):                 # nothing excluded: the counter differs
        fp.compare(parent, new, None, None)
    listed = tmp_path / "excluded.txt"
    fp.compare(parent, new, [again], str(listed))
    assert "b:screen_survivors" in listed.read_text() and "identical: 2 calls" in capsys.readouterr().out
    fp.compare(parent, new, None, None, str(listed))            # the stored list serves in place of the repeats
    for bad in ({"b": {"queries": 701}}, {"a": {"sha256": "33"}}, {"b": {"describe": "stream"}}):
        with pytest.raises(SystemExit):
            fp.compare(parent, _run(fp, tmp_path / "bad.json", **bad), [again], None)
    with pytest.raises(SystemExit):                 # two runs of one library may differ in counters only
        fp.compare(parent, new, [_run(fp, tmp_path / "p3.json", a={"sha256": "44"})], None)
