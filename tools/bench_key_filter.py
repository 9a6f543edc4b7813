#!/usr/bin/env python3
"""Per-query RANGE and IN filters (pqv.h: pqv_key_filter) against the only route the parent commit has to the same answers, and
against the existing equality window (bench.py's synth: uniform rows, seed 1234; 1024 clusters; nprobe 32; k 10; queries seed 7;
device entry points; an int32 key column uniform over 65 536 distinct keys).

(a) nq = 1024, every query its own filter -- RANGE at selectivities 1, 1/8, 1/64 (a window of 65 536 x selectivity keys at a
    random start), IN with 4, 64 and 1 024 values:
      ONE pqv_topk_filtered_device call
    against
      one prebuilt mask and one pqv_topk_masked_device call per distinct filter, all enqueued and then waited for once; the masks
      are built beforehand and not timed.  With --masked-lib PATH this route runs in a fresh child process on that library (the
      parent commit's build, which has no filtered symbols), else in this process.
(b) the cost of the new window sources over the existing one, nq in {1, 64}: RANGE with lo == hi, and IN with singletons,
    each alternating with the query_keys= call on the same keys -- ratio of the medians beside both spreads -- on the 65 536-key
    column (next to no row matches: the time is the windows') and on a one-key column (every row matches: the time is the chain's).
Times are host clock from the first enqueue to the end of a device synchronisation, medians of --reps after one warm-up.
Writes one JSON line (profiles/key_filter_bench.json is that line).
usage: python tools/bench_key_filter.py [--workload c3s|c3] [--reps N] [--masked-lib PATH]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

K, NQ, DISTINCT = 10, 1024, 65536
RANGE_SEL = (1, 8, 64)          # selectivity 1 / x
IN_LEN = (4, 64, 1024)


def stats(times):
    ms = np.asarray(times) * 1e3
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max())}


def key_column(n, distinct=DISTINCT):
    return np.random.default_rng(1000 + distinct).integers(0, distinct, n).astype(np.int32)


def range_filters(sel):
    """-> (lo, hi) int64 [NQ]: windows of DISTINCT / sel keys, inclusive"""
    width = DISTINCT // sel
    lo = np.random.default_rng(3000 + sel).integers(0, DISTINCT - width + 1, NQ).astype(np.int64)
    return lo, lo + width - 1


def set_filters(m):
    """-> (lims uint64 [NQ + 1], vals int64): NQ ascending sets of m distinct keys"""
    rng = np.random.default_rng(4000 + m)
    vals = np.concatenate([np.sort(rng.choice(DISTINCT, size=m, replace=False)) for _ in range(NQ)]).astype(np.int64)
    return np.arange(NQ + 1, dtype=np.uint64) * np.uint64(m), vals


def configs():
    for sel in RANGE_SEL:
        yield {"kind": "range", "selectivity": f"1/{sel}"}, ("range",) + range_filters(sel)
    for m in IN_LEN:
        yield {"kind": "in", "values_per_query": m}, ("in",) + set_filters(m)


def allowed_rows(column, flt, q):
    if flt[0] == "range":
        return (column >= flt[1][q]) & (column <= flt[2][q])
    member = np.zeros(DISTINCT, bool)
    member[flt[2][int(flt[1][q]):int(flt[1][q + 1])]] = True
    return member[column]


class Bench:
    def __init__(self, workload, filtered):
        import torch
        import bench
        from pq_vector_amd import _ffi
        if not filtered:      # (a library from before the filtered entry points: bind what it has)
            for name in [x for x in _ffi.SIGNATURES if "filtered" in x]:
                del _ffi.SIGNATURES[name]
        import pq_vector_amd as pqv
        self.torch, self.pqv = torch, pqv
        self.n, self.dim, kc, self.nprobe, _ = bench.WORKLOADS[workload]
        self.dev = torch.device("cuda", 0)
        self.corpus_t = bench.synth(torch, self.dev, 1234, self.n, self.dim)
        self.q_t = bench.synth(torch, self.dev, 7, NQ, self.dim)
        torch.cuda.synchronize()
        corpus = pqv.Corpus.from_device_ptr(self.corpus_t.data_ptr(), self.n, self.dim, device=0, keepalive=self.corpus_t)
        index = pqv.IndexBuilder(corpus).n_clusters(kc).max_iters(20).seed(42).workers(min(16, os.cpu_count() or 1)).build()
        self.s = pqv.Searcher(index, corpus)
        self.rows = torch.zeros((NQ, K), dtype=torch.int32, device=self.dev)
        self.dist = torch.zeros((NQ, K), dtype=torch.float32, device=self.dev)

    def timed(self, enqueue, reps):
        enqueue()
        self.torch.cuda.synchronize()
        out = []
        for _ in range(reps):
            t0 = time.perf_counter()
            enqueue()
            self.torch.cuda.synchronize()
            out.append(time.perf_counter() - t0)
        return out

    def call(self, keys, nq, **kw):
        return lambda: self.s.topk_device(self.q_t.data_ptr(), nq, K, self.nprobe, self.rows.data_ptr(), self.dist.data_ptr(), keys=keys, **kw)

    def masked_route(self, column, flt):
        """-> (enqueue, masks): one masked device call per query, each under its own prebuilt mask"""
        masks = [self.s.row_mask(allowed_rows(column, flt, q)) for q in range(NQ)]
        qp, rp, dp = self.q_t.data_ptr(), self.rows.data_ptr(), self.dist.data_ptr()
        calls = [(m, qp + 4 * self.dim * q, rp + 4 * K * q, dp + 4 * K * q) for q, m in enumerate(masks)]
        self.torch.cuda.synchronize()

        def enqueue():
            for m, q, r, d in calls:
                self.s.topk_device(q, 1, K, self.nprobe, r, d, mask=m)
        return enqueue, masks


def run_masked(b, reps):
    out = []
    column = key_column(b.n)
    for label, flt in configs():
        enqueue, masks = b.masked_route(column, flt)
        r = {**label, "nq": NQ, "route": "one masked device call per distinct filter", **stats(b.timed(enqueue, reps))}
        out.append(r)
        print(json.dumps(r), file=sys.stderr, flush=True)
        for m in masks:
            m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c3s", choices=["c3s", "c3"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--masked-lib", default=None)
    ap.add_argument("--route", default="all", choices=["all", "masked"])
    args = ap.parse_args()
    if args.route == "masked":
        print(json.dumps(run_masked(Bench(args.workload, filtered=False), args.reps)))
        return
    b = Bench(args.workload, filtered=True)
    torch, pqv = b.torch, b.pqv
    out = {"workload": args.workload, "rows": b.n, "dim": b.dim, "nprobe": b.nprobe, "k": K, "reps": args.reps, "distinct_keys": DISTINCT,
           "filtered": [], "masked_lib": args.masked_lib or "this build"}
    col = pqv.Column.upload(key_column(b.n))
    keys = b.s.row_keys(col)
    col.close()
    for label, flt in configs():
        a_t = torch.from_numpy(flt[1].view(np.int64)).to(b.dev)
        b_t = torch.from_numpy(flt[2]).to(b.dev)
        kw = {"query_key_ranges" if flt[0] == "range" else "query_key_sets": (a_t.data_ptr(), b_t.data_ptr())}
        c0 = b.s.counters()
        times = b.timed(b.call(keys, NQ, **kw), args.reps)
        c1 = b.s.counters()
        r = {**label, "nq": NQ, "route": "one filtered device call",
             "considered_rows_per_call": int((c1["embeddings_fetched"] - c0["embeddings_fetched"]) // (args.reps + 1)), **stats(times)}
        out["filtered"].append(r)
        print(json.dumps(r), file=sys.stderr, flush=True)
    if args.masked_lib:
        env = dict(os.environ, PQV_LIB_PATH=os.path.abspath(args.masked_lib))
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--route", "masked", "--workload", args.workload, "--reps", str(args.reps)],
                             env=env, stdout=subprocess.PIPE, check=True)
        out["masked"] = json.loads(res.stdout.decode().strip().splitlines()[-1])
    else:
        out["masked"] = run_masked(b, args.reps)
    out["speedup_filtered_over_masked"] = [{**{k: v for k, v in f.items() if k in ("kind", "selectivity", "values_per_query")},
                                            "speedup": m["median_ms"] / f["median_ms"]} for f, m in zip(out["filtered"], out["masked"])]
    # (b) the new window sources against the equality window, on the same keys
    out["window_cost"] = []
    one_col = pqv.Column.upload(np.zeros(b.n, np.int32))
    one_keys = b.s.row_keys(one_col)
    one_col.close()
    for distinct, kk in ((DISTINCT, keys), (1, one_keys)):
        qk = np.random.default_rng(5000 + distinct).integers(0, distinct, NQ).astype(np.int64)
        qk_t = torch.from_numpy(qk).to(b.dev)
        lims_t = torch.arange(NQ + 1, dtype=torch.int64, device=b.dev)
        for nq in (1, 64):
            eq = b.call(kk, nq, query_keys=qk_t.data_ptr())
            for name, new in (("range lo == hi", b.call(kk, nq, query_key_ranges=(qk_t.data_ptr(), qk_t.data_ptr()))),
                              ("in singletons", b.call(kk, nq, query_key_sets=(lims_t.data_ptr(), qk_t.data_ptr())))):
                t_new, t_eq = [], []
                b.timed(new, 1); b.timed(eq, 1)
                for _ in range(args.reps):
                    t_new += b.timed(new, 1)[-1:]
                    t_eq += b.timed(eq, 1)[-1:]
                r = {"distinct_keys": distinct, "nq": nq, "filter": name, "filtered": stats(t_new), "query_keys": stats(t_eq),
                     "ratio_of_medians": float(np.median(t_new) / np.median(t_eq))}
                out["window_cost"].append(r)
                print(json.dumps(r), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
