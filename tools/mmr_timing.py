#!/usr/bin/env python3
"""The MMR selection against one scoring pass over the same candidates, and the fused call beside plain top-k.

Per shape (bench.py's WORKLOADS: rows, dim, n_clusters, nprobe; bench.synth rows seed 1234 and queries seed 7; the index built on the
device with max_iters 5, seed 42) and per (k, fetch_k) in {(10, 100), (10, 256), (100, 1024)}, for 1024 queries and for one:
  stage 1      pqv_topk_device(k = fetch_k): its [nq, fetch_k] rows and distances are the candidates of what follows
  select       pqv_mmr_select_device over them, lambda 0.5: k - 1 redundancy passes of fetch_k rows each
  score        pqv_score_rows_device over the same [nq, fetch_k] lists: existing code, ONE pass over those rows -- the yardstick
  fused        pqv_topk_mmr_device, beside `plain`: pqv_topk_device(k = fetch_k)
Times are host clock from the first enqueue of `inner` back-to-back calls to the end of a device synchronisation, divided by
`inner`; medians with minimum and maximum over --reps windows after two warm windows of each; select / score and fused / plain
alternate inside one loop.  pass_over_score = select / (k - 1) / score.  The fused call's picks are compared with the selection's.
Every shape runs in a child process of its own under --timeout seconds; the first one that fails or runs out of time ends the run.
Prints one JSON line per shape.
usage: python tools/mmr_timing.py [--shapes c2,c3s] [--reps 15] [--inner 10] [--timeout 300]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAIRS = ((10, 100), (10, 256), (100, 1024))
LAMBDA = 0.5


def stats(times):
    ms = np.asarray(times) * 1e3
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max())}


def child(shape, reps, inner):
    import torch
    import bench
    import pq_vector_amd as pqv
    dev = torch.device("cuda", 0)
    n, dim, kc, nprobe, nq_max = bench.WORKLOADS[shape]
    corpus_t = bench.synth(torch, dev, 1234, n, dim)
    q_all = bench.synth(torch, dev, 7, nq_max, dim)
    torch.cuda.synchronize()
    corpus = pqv.Corpus.from_device_ptr(corpus_t.data_ptr(), n, dim, device=0, keepalive=corpus_t)
    index = pqv.IndexBuilder(corpus).max_iters(5).seed(42).workers(min(16, os.cpu_count() or 1)).n_clusters(kc).build()
    s = pqv.Searcher(index, corpus)
    out = {"shape": shape, "rows": n, "dim": dim, "n_clusters": int(index.n_clusters), "nprobe": nprobe, "lambda": LAMBDA, "reps": reps,
           "inner": inner, "cases": []}

    def window(enqueue):
        t0 = time.perf_counter()
        for _ in range(inner):
            enqueue()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / inner

    for nq in (nq_max, 1):
        q_t = q_all[:nq].contiguous()
        for k, fetch_k in PAIRS:
            i32 = lambda *shp: torch.zeros(shp, dtype=torch.int32, device=dev)      # noqa: E731
            f32 = lambda *shp: torch.zeros(shp, dtype=torch.float32, device=dev)    # noqa: E731
            c_rows, c_dist, c_nf, c_nc = i32(nq, fetch_k), f32(nq, fetch_k), i32(nq), torch.zeros(nq, dtype=torch.int64, device=dev)
            s_rows, s_dist, s_score, s_nf = i32(nq, k), f32(nq, k), f32(nq, k), i32(nq)
            f_rows, f_dist, f_score, f_nf, f_nc = i32(nq, k), f32(nq, k), f32(nq, k), i32(nq), torch.zeros(nq, dtype=torch.int64, device=dev)
            sc_dist = f32(nq * fetch_k)
            lims_t = (torch.arange(nq + 1, dtype=torch.int64, device=dev) * fetch_k).contiguous()

            def plain():
                s.topk_device(q_t.data_ptr(), nq, fetch_k, nprobe, c_rows.data_ptr(), c_dist.data_ptr(), c_nf.data_ptr(), c_nc.data_ptr())

            def select():
                s.mmr_select_device(c_rows.data_ptr(), c_dist.data_ptr(), nq, fetch_k, k, s_rows.data_ptr(), s_dist.data_ptr(),
                                    s_score.data_ptr(), s_nf.data_ptr(), d_n_found_in=c_nf.data_ptr(), lambda_=LAMBDA)

            def score():
                s.score_rows_device(q_t.data_ptr(), nq, lims_t.data_ptr(), c_rows.data_ptr(), sc_dist.data_ptr())

            def fused():
                s.topk_mmr_device(q_t.data_ptr(), nq, k, fetch_k, nprobe, f_rows.data_ptr(), f_dist.data_ptr(), f_score.data_ptr(),
                                  f_nf.data_ptr(), f_nc.data_ptr(), lambda_=LAMBDA)

            plain()
            torch.cuda.synchronize()
            for _ in range(2):
                for call in (select, score, fused, plain):
                    window(call)
            t = {"select": [], "score": [], "fused": [], "plain": []}
            for _ in range(reps):
                for name, call in (("select", select), ("score", score), ("fused", fused), ("plain", plain)):
                    t[name].append(window(call))
            equal = all(bool((a == b).all()) for a, b in ((s_rows, f_rows), (s_dist, f_dist), (s_score, f_score), (s_nf, f_nf)))
            med = {name: float(np.median(v)) for name, v in t.items()}
            r = {"nq": nq, "k": k, "fetch_k": fetch_k, "found_min": int(c_nf.min()), "picks_min": int(s_nf.min()), "fused_equals_select": equal,
                 **{name: stats(v) for name, v in t.items()},
                 "pass_us": med["select"] / (k - 1) * 1e6, "pass_over_score": med["select"] / (k - 1) / med["score"],
                 "fused_minus_plain_ms": (med["fused"] - med["plain"]) * 1e3}
            out["cases"].append(r)
            print(json.dumps(r), file=sys.stderr, flush=True)
    s.close()
    index.close()
    corpus.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,c3s")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=300, help="seconds one shape's child process may take")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.reps, args.inner)
        return 0
    for shape in args.shapes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", shape, "--reps", str(args.reps), "--inner", str(args.inner)]
        try:
            rc = subprocess.run(cmd, timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            print(f"{shape}: no result within {args.timeout} s; nothing further is started", file=sys.stderr)
            return 124
        if rc != 0:
            print(f"{shape}: the measurement ended with status {rc}; nothing further is started", file=sys.stderr)
            return rc if rc > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
