#!/usr/bin/env python3
"""Per-query key filters against today's only route to the same answers (bench.py's synth: uniform rows, seed 1234; 1024
clusters; nprobe 32; k 10; queries seed 7; device entry points; keys uniform over T tenants, int32).

T in {16, 1024, 65536}, nq = 1024:
  (a) ONE pqv_topk_keyed_device call;
  (b) the same queries grouped by key, one pqv_topk_masked_device call per distinct key, all enqueued and then waited for once;
      the masks are built beforehand and not timed.  With --masked-lib PATH route (b) runs in a child process on that library (the
      parent commit's build, which has no keyed symbols), else in this process.
T = 1 (every row matches), nq in {1, 64}: the keyed call alternating with the masked all-ones call -- ratio of the medians and the
run-to-run spread -- beside the byte ratio (4 dim + key bytes) / (4 dim + 1/8).
Times are host clock from the first enqueue to the end of a device synchronisation, medians of --reps after one warm-up.
Writes one JSON line (profiles/keyed_bench.json is that line).
usage: python tools/bench_keyed.py [--workload c3s|c3] [--reps N] [--masked-lib PATH]"""
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

K, NQ, TENANTS = 10, 1024, (16, 1024, 65536)


def stats(times):
    ms = np.asarray(times) * 1e3
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max())}


def tenant_column(n, t):
    return np.random.default_rng(1000 + t).integers(0, t, n).astype(np.int32)


def query_keys(n_q, t):
    return np.random.default_rng(2000 + t).integers(0, t, n_q).astype(np.int64)


class Bench:
    def __init__(self, workload, keyed):
        import torch
        import bench
        from pq_vector_amd import _ffi
        if not keyed:      # (a library from before the keyed entry points: bind what it has)
            for name in [x for x in _ffi.SIGNATURES if "keyed" in x or "row_keys" in x]:
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

    def keyed_call(self, keys, qk_t, nq):
        return lambda: self.s.topk_device(self.q_t.data_ptr(), nq, K, self.nprobe, self.rows.data_ptr(), self.dist.data_ptr(),
                                          keys=keys, query_keys=qk_t.data_ptr())

    def masked_groups(self, column, qkeys):
        """-> (enqueue, masks, distinct keys): one masked device call per distinct key over that key's queries"""
        torch = self.torch
        groups = {}
        for i, key in enumerate(qkeys.tolist()):
            groups.setdefault(key, []).append(i)
        calls, masks, keep = [], [], []
        at = 0
        for key, idx in groups.items():
            m = self.s.row_mask(column == key)
            q = self.q_t[torch.tensor(idx, device=self.dev)].contiguous()
            masks.append(m); keep.append(q)
            calls.append((m, q.data_ptr(), len(idx), self.rows[at:at + len(idx)].data_ptr(), self.dist[at:at + len(idx)].data_ptr()))
            at += len(idx)
        torch.cuda.synchronize()

        def enqueue():
            for m, qp, nq, rp, dp in calls:
                self.s.topk_device(qp, nq, K, self.nprobe, rp, dp, mask=m)
        enqueue.keep = keep
        return enqueue, masks, len(groups)


def run_masked(b, reps):
    out = []
    for t in TENANTS:
        enqueue, masks, distinct = b.masked_groups(tenant_column(b.n, t), query_keys(NQ, t))
        r = {"tenants": t, "nq": NQ, "distinct_keys": distinct, "route": "one masked device call per distinct key", **stats(b.timed(enqueue, reps))}
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
        print(json.dumps(run_masked(Bench(args.workload, keyed=False), args.reps)))
        return
    b = Bench(args.workload, keyed=True)
    torch, pqv = b.torch, b.pqv
    out = {"workload": args.workload, "rows": b.n, "dim": b.dim, "nprobe": b.nprobe, "k": K, "reps": args.reps, "keyed": [],
           "masked_lib": args.masked_lib or "this build"}
    for t in TENANTS:
        col = pqv.Column.upload(tenant_column(b.n, t))
        t0 = time.perf_counter()
        keys = b.s.row_keys(col)
        create_ms = (time.perf_counter() - t0) * 1e3
        col.close()
        qk_t = torch.from_numpy(query_keys(NQ, t)).to(b.dev)
        c0 = b.s.counters()
        times = b.timed(b.keyed_call(keys, qk_t, NQ), args.reps)
        c1 = b.s.counters()
        considered = (c1["embeddings_fetched"] - c0["embeddings_fetched"]) // (args.reps + 1)
        r = {"tenants": t, "nq": NQ, "route": "one keyed device call", "row_keys_create_ms": create_ms,
             "considered_rows_per_call": int(considered), **stats(times)}
        out["keyed"].append(r)
        print(json.dumps(r), file=sys.stderr, flush=True)
        keys.close()
    if args.masked_lib:
        env = dict(os.environ, PQV_LIB_PATH=os.path.abspath(args.masked_lib))
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--route", "masked", "--workload", args.workload, "--reps", str(args.reps)],
                             env=env, stdout=subprocess.PIPE, check=True)
        out["masked"] = json.loads(res.stdout.decode().strip().splitlines()[-1])
    else:
        out["masked"] = run_masked(b, args.reps)
    out["speedup_keyed_over_masked"] = {str(a["tenants"]): m["median_ms"] / a["median_ms"] for a, m in zip(out["keyed"], out["masked"])}
    # T = 1: every row matches -- the keyed call alternating with the masked all-ones call
    col = pqv.Column.upload(np.zeros(b.n, np.int32))
    keys = b.s.row_keys(col)
    col.close()
    ones = b.s.row_mask(np.ones(b.n, bool))
    qk_t = torch.zeros(NQ, dtype=torch.int64, device=b.dev)
    out["all_rows_match"] = []
    for nq in (1, 64):
        keyed = b.keyed_call(keys, qk_t, nq)

        def masked():
            b.s.topk_device(b.q_t.data_ptr(), nq, K, b.nprobe, b.rows.data_ptr(), b.dist.data_ptr(), mask=ones)
        t_k, t_m = [], []
        b.timed(keyed, 1); b.timed(masked, 1)
        for _ in range(args.reps):
            t_k += b.timed(keyed, 1)[-1:]
            t_m += b.timed(masked, 1)[-1:]
        r = {"nq": nq, "keyed": stats(t_k), "masked_all_ones": stats(t_m),
             "ratio_of_medians": float(np.median(t_k) / np.median(t_m)),
             "byte_ratio": (4 * b.dim + 4) / (4 * b.dim + 0.125)}
        out["all_rows_match"].append(r)
        print(json.dumps(r), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
