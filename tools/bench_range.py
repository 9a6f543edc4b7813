#!/usr/bin/env python3
"""pqv_range_search on C3 (bench.py's synth: 10 M x 768 uniform, seed 1234; 1024 clusters; nprobe 32; queries seed 7).

Radii are taken from query 0's sorted candidate distances: its 10th and 100th nearest and its 1 % quantile (about 10, 100
and 1 % of the candidates per query).  For nq = 1 and nq = 1024 at each radius: call time (host clock around the
synchronous call), the library's hipEvent times (pqv_set_timing: the STREAM_RANGE pass, and probe .. write-out), the
stream pass's f32 bytes (capped candidates x 4 dim) and their fraction of 8 TB/s.  The only other way to the same answer,
pqv_topk with k = the batch's largest candidate count plus a host filter, is timed on a few queries of the batch (that path
runs one query at a time) and scaled to the batch.  Prints one JSON line.
usage: python tools/bench_range.py [--reps N] [--baseline-queries M] [--no-baseline]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-queries", type=int, default=8)
    ap.add_argument("--no-baseline", action="store_true")
    args = ap.parse_args()
    import torch
    import bench
    import pq_vector_amd as pqv
    n, dim, kc, nprobe, nq = bench.WORKLOADS["c3"]
    dev = torch.device("cuda", 0)
    corpus_t = bench.synth(torch, dev, 1234, n, dim)
    queries = bench.synth(torch, dev, 7, nq, dim).cpu().numpy()
    torch.cuda.synchronize()
    corpus = pqv.Corpus.from_device_ptr(corpus_t.data_ptr(), n, dim, device=0, keepalive=corpus_t)
    index = pqv.IndexBuilder(corpus).n_clusters(kc).max_iters(20).seed(42).workers(os.cpu_count() or 1).build()
    s = pqv.Searcher(index, corpus)
    _, _, d0, _, nc0 = s.range_search(queries[:1], float("inf"), nprobe)
    radii = {"10_hits": float(d0[9]), "100_hits": float(d0[99]), "1pct": float(d0[len(d0) // 100])}
    out = {"workload": "c3", "rows": n, "dim": dim, "n_clusters": kc, "nprobe": nprobe,
           "query0_candidates": int(nc0[0]), "radii": radii, "hbm_peak_TBps": 8.0, "configs": []}
    for name, r in radii.items():
        for b in (1, nq):
            qs = queries[:b]
            res = s.range_search(qs, r, nprobe)                     # warm-up (scratch sized, code loaded)
            s.timing_read()
            s.set_timing(True)
            times = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                res = s.range_search(qs, r, nprobe)
                times.append(time.perf_counter() - t0)
            s.set_timing(False)
            stream_ms, total_ms, calls = s.timing_read()
            lims, _, _, nw, nc = res
            capped = int(nc.sum())
            bytes_ = capped * 4 * dim
            # (the library records one event set per sub-batch: per call = the sums over the repetitions)
            stream_s = stream_ms / 1e3 / args.reps
            out["configs"].append({
                "radius_for": name, "radius": r, "nq": b,
                "hits_per_query": float(nw.mean()), "hit_fraction": float(nw.sum() / max(1, capped)),
                "call_ms_median": float(np.median(times) * 1e3), "call_ms_min": float(np.min(times) * 1e3),
                "stream_kernel_ms": stream_s * 1e3, "device_span_ms": total_ms / args.reps, "sub_batches": calls // args.reps,
                "stream_bytes": bytes_, "stream_TBps": bytes_ / stream_s / 1e12 if stream_s else None,
                "stream_frac_of_8TBps": bytes_ / stream_s / 8e12 if stream_s else None,
                "q_per_s": b / float(np.median(times)),
            })
            print(json.dumps(out["configs"][-1]), file=sys.stderr, flush=True)
    if not args.no_baseline:
        # today's only route to the same answer: pqv_topk with k = the batch's largest capped candidate count (every
        # candidate comes back sorted), then keep the prefix within the radius on the host
        r = radii["1pct"]
        _, _, _, _, nc = s.range_search(queries, r, nprobe)
        k = int(nc.max())
        m = args.baseline_queries
        t0 = time.perf_counter()
        for i in range(m):
            rows, dist, nf, _ = s.topk(queries[i:i + 1], k, nprobe)
            keep = dist[0, :nf[0]] <= np.float32(r)
            _ = rows[0, :nf[0]][keep]
        per_q = (time.perf_counter() - t0) / m
        t0 = time.perf_counter()
        s.range_search(queries, r, nprobe)
        range_s = time.perf_counter() - t0
        out["baseline_topk_filter"] = {"k": k, "queries_timed": m, "s_per_query": per_q, "s_for_batch_scaled": per_q * nq,
                                       "range_search_batch_s": range_s, "speedup": per_q * nq / range_s}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
