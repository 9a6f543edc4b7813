#!/usr/bin/env python3
"""Fingerprint of the host dispatch: a fixed list of search calls over small seeded indexes, each in a process of its own, each
printing a SHA-256 of everything it returned, the pqv_counters delta and the pqv_searcher_describe string.  Two builds of the
library that route, launch and compute alike print the same file.

    PQV_LIB_PATH=/path/to/libpqv_hip.so python tools/route_fingerprint.py --out run.json      # one run (needs a GPU)
    python tools/route_fingerprint.py --compare parent.json new.json --self parent_again.json [...] --excluded-out excluded.txt
    python tools/route_fingerprint.py --compare parent.json new.json --excluded-in excluded.txt

Every case names the route it is there for (`expect`: substrings of the describe string; request kinds: the call succeeds and
finds rows); a shape that quietly falls onto another path fails its case.  --compare drops the counters that differ between two
runs of the SAME library (--self: the screened paths' running thresholds make what they fetch depend on block order), lists
them by name, and demands that everything else is identical."""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


# ---------------------------------------------------------------------------------------------------------------------------
# seeded data: clustered rows, the generating centres as centroids, each centre's rows as its list
# ---------------------------------------------------------------------------------------------------------------------------
def clustered(seed, dim, sizes):
    rng = np.random.default_rng(seed)
    kc = len(sizes)
    cen = (rng.standard_normal((kc, dim)) * 2.0).astype(np.float32)
    owner = rng.permutation(np.repeat(np.arange(kc), sizes))
    data = (cen[owner] + 0.3 * rng.standard_normal((len(owner), dim))).astype(np.float32)
    lists = [np.flatnonzero(owner == c).astype(np.uint32) for c in range(kc)]
    return rng, cen, np.ascontiguousarray(data), lists


def near_queries(rng, cen, nq, pop=None, spread=0.4):
    c = rng.choice(len(cen), size=nq, p=pop)
    return (cen[c] + spread * rng.standard_normal((nq, cen.shape[1]))).astype(np.float32)


POP9 = np.array([0.45, 0.2, 0.12, 0.08, 0.06, 0.04, 0.03, 0.015, 0.005])
SIZES9 = [4001, 2977, 1500, 833, 700, 650, 517, 300, 45]
DATASETS = {                         # name -> (seed, dim, list sizes)
    "s32": (1, 32, [400, 112] * 8),             # rows of 32 dims, unequal lists: the exact stream and the older tile forms
    "pad100": (2, 100, [256] * 16),             # stored zero-padded to 128 dims
    "w256": (3, 256, SIZES9),                   # every wide-screen operand; popular lists for the wide-quad instance
    "g320": (4, 320, [512] * 8),                # f32 operands, a quad's queries too long for LDS
    "many": (5, 32, [4] * 1100),                # more than 1024 lists: the host probe of range search
}


class Dev:
    """Device buffers through the HIP runtime the library itself is linked against (no second runtime in the process)."""

    def __init__(self, lib):
        self.hip = lib
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        self.bufs = []

    def _ok(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed with HIP error {rc}")

    def zeros(self, nbytes):
        p = C.c_void_p()
        self._ok(self.hip.hipMalloc(C.byref(p), max(8, nbytes)), "hipMalloc")
        self._ok(self.hip.hipMemset(p, 0, max(8, nbytes)), "hipMemset")
        self.bufs.append(p)
        return p.value

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = self.zeros(a.nbytes)
        if a.nbytes:
            self._ok(self.hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1), "hipMemcpy to the device")
        return p

    def get(self, p, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        self._ok(self.hip.hipDeviceSynchronize(), "hipDeviceSynchronize")
        if out.nbytes:
            self._ok(self.hip.hipMemcpy(out.ctypes.data, p, out.nbytes, 2), "hipMemcpy to the host")
        return out

    def sync(self):
        self._ok(self.hip.hipDeviceSynchronize(), "hipDeviceSynchronize")


# ---------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------
def case(name, data, kind="topk", form="host", nq=8, k=10, nprobe=4, opts=None, expect=(), **kw):
    return dict(name=name, data=data, kind=kind, form=form, nq=nq, k=k, nprobe=nprobe, opts=opts or {}, expect=tuple(expect), **kw)


STREAM = ("stream_kernel: one candidate stream",)
SCREEN = {"rerank_mode": 2, "tile_filter": 2}


def cases():
    out = []
    for form in ("host", "device"):
        f = "" if form == "host" else "_device"
        out += [case(f"plain_k10{f}", "s32", form=form, expect=STREAM),
                case(f"plain_k100{f}", "s32", form=form, k=100, expect=STREAM),
                case(f"plain_k300{f}", "s32", form=form, k=300, expect=STREAM),
                case(f"dot{f}", "s32", form=form, metric="dot", expect=("PQV_DOT: dot_stream_kernel",)),
                case(f"cosine{f}", "s32", form=form, metric="cosine", expect=("PQV_COSINE",)),
                case(f"masked{f}", "s32", form=form, mask=0.5)]
        for filt in ("eq", "range", "in"):
            for width in ("i32", "i64"):
                for m in (None, 0.5):
                    out.append(case(f"keyed_{filt}_{width}{'_mask' if m else ''}{f}", "s32", form=form, keys=width, filt=filt, mask=m))
        out += [case(f"expand_mask{f}", "s32", form=form, nprobe=1, mask=0.02, max_nprobe=8),
                case(f"expand_filter{f}", "s32", form=form, nprobe=1, keys="i64", filt="eq", max_nprobe=8),
                case(f"distinct{f}", "s32", kind="distinct", form=form, group="i32"),
                case(f"grouped_m1{f}", "s32", kind="grouped", form=form, group="i64", group_size=1),
                case(f"grouped_m3{f}", "s32", kind="grouped", form=form, group="i32", group_size=3),
                case(f"distinct_filtered{f}", "s32", kind="distinct", form=form, group="i32", keys="i64", filt="range"),
                case(f"grouped_filtered{f}", "s32", kind="grouped", form=form, group="i64", group_size=3, keys="i32", filt="in"),
                case(f"distinct_expand{f}", "s32", kind="distinct", form=form, group="i32", nprobe=1, mask=0.02, max_nprobe=8),
                case(f"grouped_expand{f}", "s32", kind="grouped", form=form, group="i32", group_size=2, nprobe=1, keys="i64", filt="eq",
                     max_nprobe=8)]
    out += [case("table_cap", "s32", table=True, nprobe=2, max_candidates=300, expect=("table of 2 files",)),
            case("tile_rerank", "s32", nq=64, expect=("tile_rerank_kernel: exact arithmetic",)),
            case("tile_filter_f32", "s32", nq=64, opts=SCREEN, expect=("tile_filter_kernel: 16-query groups, f32 screen operands",)),
            case("padded", "pad100", nq=64, expect=("rows stored zero-padded from 100 to 128 dims", "wide_filter_kernel")),
            case("q_global", "g320", nq=64, nprobe=3, expect=("f32 screen operands", "as a blocked copy in global memory")),
            case("deferred", "w256", nq=700, k=100, nprobe=3, pop=True, opts=SCREEN, expect=("exact evaluations deferred",))]
    for op, o in (("i8", {}), ("f16", {"screen_i8": 0}), ("f32", {"screen_i8": 0, "screen_f16": 0})):
        name = {"i8": "int8", "f16": "f16", "f32": "f32"}[op] + " screen operands"
        wide = ("lists probed by 97..160 queries: one quad",) if op == "i8" else ()
        out += [case(f"wide_{op}_one", "w256", nq=1, nprobe=3, opts={**SCREEN, **o}, expect=(name, ", 12>; seed_select_kernel")),
                case(f"wide_{op}_batch", "w256", nq=700, nprobe=3, pop=True, opts={**SCREEN, **o}, expect=(name, "staged in LDS") + wide)]
    out += [case("range", "s32", kind="range", radius=2.9),
            case("range_masked", "s32", kind="range", radius=2.9, mask=0.5),
            case("range_dot", "s32", kind="range", radius=-100.0, metric="dot"),
            case("range_host_probe", "many", kind="range", radius=2.9, nprobe=1100)]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# one case, in this process
# ---------------------------------------------------------------------------------------------------------------------------
def run_case(c):
    import pq_vector_amd as pqv
    from pq_vector_amd import _ffi
    seed, dim, sizes = DATASETS[c["data"]]
    rng, cen, data, lists = clustered(seed, dim, sizes)
    n = len(data)
    nq, k, nprobe = c["nq"], c["k"], c["nprobe"]
    queries = near_queries(rng, cen, nq, POP9 if c.get("pop") else None)
    metric = {"dot": _ffi.PQV_DOT, "cosine": _ffi.PQV_COSINE}.get(c.get("metric"), _ffi.PQV_L2SQ_REF4)
    corpus = pqv.Corpus.upload(data)
    if c.get("table"):              # two files: the lists' rows below / from n // 2, each file's rows local to it
        half = n // 2
        ixs = [pqv.Index.from_parts(dim, cen, [l[l < half] for l in lists]),
               pqv.Index.from_parts(dim, cen, [l[l >= half] - half for l in lists])]
        s = pqv.TableSearcher(ixs, corpus, [0, half], flags=_ffi.PQV_LAYOUT_IVF_ORDERED | _ffi.PQV_TABLE_CAP_ROUND_ROBIN)
    else:
        s = pqv.Searcher(pqv.Index.from_parts(dim, cen, lists), corpus)
    for name, value in c["opts"].items():
        s.set_option(name, value)
    dev = Dev(_ffi.lib())
    device = c["form"] == "device"

    def column(width, mod, nulls):
        vals = (np.arange(n) * 7 % mod).astype(np.int32 if width == "i32" else np.int64)
        valid = (np.arange(n) % 11 != 0).astype(np.uint8) if nulls else None
        return s.row_keys(pqv.Column.upload(vals, valid))

    kw = {}
    if c.get("mask"):
        kw["mask"] = s.row_mask(rng.random(n) < c["mask"])
    if c.get("keys"):                        # 64 tenants; the i64 column has NULLs
        kw["filter_keys" if c["kind"] != "topk" and c["kind"] != "range" else "keys"] = column(c["keys"], 64, c["keys"] == "i64")
        qk = (np.arange(nq) % 64).astype(np.int64)
        if c["filt"] == "eq":
            kw["query_keys"] = dev.put(qk) if device else qk
        elif c["filt"] == "range":
            lo, hi = qk, qk + 2
            kw["query_key_ranges"] = (dev.put(lo), dev.put(hi)) if device else (lo, hi)
        else:
            sets = [sorted({int(v), int((v + 3) % 64), int((v + 5) % 64)}) for v in qk]
            if device:
                lims = np.concatenate([[0], np.cumsum([len(x) for x in sets])]).astype(np.uint64)
                kw["query_key_sets"] = (dev.put(lims), dev.put(np.concatenate(sets).astype(np.int64)))
            else:
                kw["query_key_sets"] = sets
    if c.get("group"):                       # documents of 4 rows; the i64 column has NULLs
        vals = (np.arange(n) // 4).astype(np.int32 if c["group"] == "i32" else np.int64)
        valid = (np.arange(n) % 11 != 0).astype(np.uint8) if c["group"] == "i64" else None
        group = s.row_keys(pqv.Column.upload(vals, valid))
    if c.get("max_nprobe"):
        kw["max_nprobe"] = c["max_nprobe"]
    if c.get("max_candidates"):
        kw["max_candidates"] = c["max_candidates"]
    m = c.get("group_size", 0)

    describe = s.describe(nq, k, nprobe, metric)
    for want in c["expect"]:
        if want not in describe:
            raise AssertionError(f"{c['name']}: the dispatch does not say {want!r}: {describe}")
    before = s.counters()
    if c["kind"] == "range":
        kw.pop("max_nprobe", None)
        out = s.range_search(queries, c["radius"], nprobe, metric=metric, **kw)
        names = ["lims", "rows", "dist", "n_within", "n_candidates"]
        found = int(out[0][-1])
    elif not device:
        if c["kind"] == "topk":
            out = s.topk(queries, k, nprobe, metric=metric, **kw)
            names = ["rows", "dist", "n_found", "n_candidates", "nprobe_used"]
        elif c["kind"] == "distinct":
            out = s.topk_distinct(queries, k, nprobe, group, metric=metric, **kw)
            names = ["rows", "dist", "group_keys", "n_found", "n_candidates", "nprobe_used"]
        else:
            out = s.topk_grouped(queries, k, m, nprobe, group, metric=metric, **kw)
            names = ["rows", "dist", "group_keys", "group_rows", "n_found", "n_candidates", "nprobe_used"]
        found = int(out[names.index("n_found")].sum())
    else:
        km = k * max(1, m)
        d_q = dev.put(queries)
        d = {"rows": (dev.zeros(nq * km * 4), (nq, km), np.uint32), "dist": (dev.zeros(nq * km * 4), (nq, km), np.float32),
             "n_found": (dev.zeros(nq * 4), (nq,), np.uint32), "n_candidates": (dev.zeros(nq * 8), (nq,), np.uint64)}
        if c["kind"] != "topk":
            d["group_keys"] = (dev.zeros(nq * k * 8), (nq, k), np.int64)
        if c["kind"] == "grouped":
            d["group_rows"] = (dev.zeros(nq * k * 4), (nq, k), np.uint32)
        if c.get("max_nprobe"):
            d["nprobe_used"] = (dev.zeros(nq * 4), (nq,), np.uint32)
            kw["d_nprobe_used"] = d["nprobe_used"][0]
        dev.sync()
        common = dict(d_n_found=d["n_found"][0], d_n_candidates=d["n_candidates"][0], metric=metric, **kw)
        if c["kind"] == "topk":
            s.topk_device(d_q, nq, k, nprobe, d["rows"][0], d["dist"][0], **common)
        elif c["kind"] == "distinct":
            s.topk_distinct_device(d_q, nq, k, nprobe, group, d["rows"][0], d["dist"][0], d_group_key=d["group_keys"][0], **common)
        else:
            s.topk_grouped_device(d_q, nq, k, m, nprobe, group, d["rows"][0], d["dist"][0], d_group_key=d["group_keys"][0],
                                  d_group_rows=d["group_rows"][0], **common)
        names = sorted(d)
        out = [dev.get(*d[x]) for x in names]
        found = int(out[names.index("n_found")].sum())
    after = s.counters()
    if found == 0:
        raise AssertionError(f"{c['name']}: the call found nothing")
    if c.get("max_nprobe"):
        used = out[names.index("nprobe_used")]
        if not (used > nprobe).any():
            raise AssertionError(f"{c['name']}: no query probed past nprobe = {nprobe}: {used}")
    h = hashlib.sha256()
    for name, a in zip(names, out):
        a = np.ascontiguousarray(a)
        h.update(f"{name}:{a.dtype}:{a.shape};".encode())
        h.update(a.tobytes())
    return {"call": c["name"], "sha256": h.hexdigest(), "counters": {x: after[x] - before[x] for x in after}, "describe": describe}


# ---------------------------------------------------------------------------------------------------------------------------
# driver and comparison
# ---------------------------------------------------------------------------------------------------------------------------
def write_results(path, results):
    """One line per call, counters that did not move left out; the describe strings, which many calls share, once each under an id."""
    texts = sorted({r["describe"] for r in results})
    ids = {t: f"d{i}" for i, t in enumerate(texts)}
    with open(path, "w") as f:
        f.write('{"describe": {\n' + ",\n".join(f" {json.dumps(ids[t])}: {json.dumps(t)}" for t in texts) + '\n},\n"calls": [\n')
        f.write(",\n".join(" " + json.dumps({**r, "describe": ids[r["describe"]], "counters": {k: v for k, v in r["counters"].items() if v}},
                                        sort_keys=True) for r in results) + "\n]}\n")


def load_results(path):
    d = json.load(open(path))
    names = sorted({k for r in d["calls"] for k in r["counters"]})
    return {r["call"]: {**r, "describe": d["describe"][r["describe"]], "counters": {k: r["counters"].get(k, 0) for k in names}} for r in d["calls"]}


def run_all(out_path, timeout, only, keep_going):
    results, failed = [], []
    for c in cases():
        if only and c["name"] not in only:
            continue
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--call", c["name"]], capture_output=True, text=True,
                               timeout=timeout)
        except subprocess.TimeoutExpired:
            sys.exit(f"{c['name']}: no answer within {timeout} s; stopping (nothing more is started on the GPU)")
        if r.returncode == 1 and keep_going:      # (a Python exception: a case that missed its route, not a fault)
            print(f"{c['name']}: FAILED: {r.stderr.strip().splitlines()[-1] if r.stderr.strip() else ''}", flush=True)
            failed.append(c["name"])
            continue
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"{c['name']}: exit status {r.returncode}; stopping (nothing more is started on the GPU)")
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(f"{c['name']}: ok", flush=True)
        write_results(out_path, results)        # (rewritten after every call: a stopped run leaves what it had)
    print(f"{len(results)} calls -> {out_path}")
    if failed:
        sys.exit("failed: " + " ".join(failed))


def compare(a_path, b_path, self_paths, excluded_out, excluded_in=None):
    load = load_results
    a, b = load(a_path), load(b_path)
    excluded = [x.strip() for x in open(excluded_in) if x.strip() and not x.startswith("#")] if excluded_in else []
    for self_path in self_paths or []:         # (a repeat may hold some of the calls only: --only)
        a2 = load(self_path)
        for name in a2:
            if name not in a or a[name]["sha256"] != a2[name]["sha256"] or a[name]["describe"] != a2[name]["describe"]:
                sys.exit(f"{name}: two runs of the same library differ in more than a counter")
            excluded += [f"{name}:{x}" for x in a[name]["counters"]
                         if a[name]["counters"][x] != a2[name]["counters"][x] and f"{name}:{x}" not in excluded]
    if excluded_out:
        with open(excluded_out, "w") as f:
            f.write("# counters that differ between two runs of the same library (call:counter), excluded from the comparison\n")
            f.write("".join(x + "\n" for x in excluded))
    print("excluded counters:", ", ".join(excluded) if excluded else "none")
    bad = []
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            bad.append(f"{name}: in one file only")
            continue
        for field in ("sha256", "describe"):
            if a[name][field] != b[name][field]:
                bad.append(f"{name}: {field} differs: {a[name][field]!r} != {b[name][field]!r}")
        for x in a[name]["counters"]:
            if f"{name}:{x}" not in excluded and a[name]["counters"][x] != b[name]["counters"].get(x):
                bad.append(f"{name}: counter {x}: {a[name]['counters'][x]} != {b[name]['counters'].get(x)}")
    if bad:
        sys.exit("\n".join(bad))
    print(f"identical: {len(a)} calls")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", help="run every call, each in a process of its own, and write their lines here")
    ap.add_argument("--call", help="run this one call in this process and print its line")
    ap.add_argument("--only", nargs="*", help="with --out: these calls only")
    ap.add_argument("--timeout", type=float, default=120.0, help="seconds per call")
    ap.add_argument("--keep-going", action="store_true", help="with --out: go on after a call that raised (never after a signal or a timeout)")
    ap.add_argument("--list", action="store_true")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    ap.add_argument("--self", dest="self_paths", nargs="+", help="further runs of A's library: counters that differ from A are excluded")
    ap.add_argument("--excluded-out", help="write the excluded counters here, one call:counter per line")
    ap.add_argument("--excluded-in", help="a list written by --excluded-out, in place of (or on top of) --self")
    a = ap.parse_args()
    if a.list:
        print("\n".join(c["name"] for c in cases()))
    elif a.call:
        c = [x for x in cases() if x["name"] == a.call]
        if not c:
            sys.exit(f"no call named {a.call}")
        print(json.dumps(run_case(c[0]), sort_keys=True))
    elif a.compare:
        compare(a.compare[0], a.compare[1], a.self_paths, a.excluded_out, a.excluded_in)
    elif a.out:
        run_all(a.out, a.timeout, a.only, a.keep_going)
    else:
        ap.print_help()


if __name__ == "__main__":
    main()
