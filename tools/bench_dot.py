#!/usr/bin/env python3
"""PQV_DOT through the index (include/pqv.h: PQV_DOT), measured; writes profiles/dot_c3_bench.json.

bench.py's C3 shape (10 M x 768 uniform, seed 1234; 1024 clusters; nprobe 32; k 10; queries seed 7), or --rows N of it.  For one
query and for 64 queries the DOT call (dot_stream_kernel: always the exact stream) alternates with the SAME searcher's
PQV_L2SQ_REF4 call forced onto the exact stream (rerank_mode = 1: stream_kernel).  Two probe widths: C3's nprobe 32, where the
two metrics probe DIFFERENT lists (on uniform rows the largest inner products belong to the few centroids of largest norm, whose
lists are short: far fewer considered rows than the L2 call -- the record says how many), and nprobe = n_clusters ("all_lists"),
where both passes read exactly the same rows, so the expectation is a time ratio of about 1.  Per alternation: host-clock call
time around a synchronised pqv_topk_device call and the re-rank pass from pqv_set_timing; per metric: the medians, considered
rows x 4 dim bytes over the re-rank time, and the DOT / L2 ratio of every alternation with its spread.

usage: python tools/bench_dot.py [--rows N] [--alternations N] [--calls N] [--out PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def timed_calls(torch, s, st, q_t, k, nprobe, metric, calls):
    """-> (median call s, median re-rank ms, considered rows per call)"""
    nq = q_t.shape[0]
    dev = q_t.device
    r_t = torch.empty((nq, k), dtype=torch.int32, device=dev)
    d_t = torch.empty((nq, k), dtype=torch.float32, device=dev)
    wall, rr = [], []
    c0 = s.counters()["embeddings_fetched"]
    for _ in range(calls):
        st.synchronize()
        t0 = time.perf_counter()
        s.topk_device(q_t.data_ptr(), nq, k, nprobe, r_t.data_ptr(), d_t.data_ptr(), metric=metric, sqrt_out=False, stream=st.cuda_stream)
        st.synchronize()
        wall.append(time.perf_counter() - t0)
        rerank_ms, _, n = s.timing_read()
        rr.append(rerank_ms / max(1, n))
    rows = (s.counters()["embeddings_fetched"] - c0) / calls
    return float(np.median(wall)), float(np.median(rr)), rows


def shape(torch, pqv, s, st, q_t, k, nprobe, dim, alternations, calls):
    out = {"queries": int(q_t.shape[0]), "nprobe": nprobe, "calls_per_alternation": calls, "alternations": []}
    for metric in (pqv.PQV_DOT, pqv.PQV_L2SQ_REF4):                      # warm-up: scratch lanes, code objects
        timed_calls(torch, s, st, q_t, k, nprobe, metric, 3)
    for _ in range(alternations):
        rec = {}
        for name, metric in (("dot", pqv.PQV_DOT), ("l2_stream", pqv.PQV_L2SQ_REF4)):
            wall, rr, rows = timed_calls(torch, s, st, q_t, k, nprobe, metric, calls)
            rec[name] = {"call_us": wall * 1e6, "rerank_ms": rr, "considered_rows": rows,
                         "rerank_GBps": rows * 4 * dim / (rr * 1e-3) / 1e9 if rr > 0 else None}
        rec["dot_over_l2_call"] = rec["dot"]["call_us"] / rec["l2_stream"]["call_us"]
        rec["dot_over_l2_rerank"] = rec["dot"]["rerank_ms"] / rec["l2_stream"]["rerank_ms"] if rec["l2_stream"]["rerank_ms"] > 0 else None
        out["alternations"].append(rec)
    for key in ("dot_over_l2_call", "dot_over_l2_rerank"):
        v = [a[key] for a in out["alternations"] if a[key] is not None]
        out[key] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} if v else None
    for name in ("dot", "l2_stream"):
        v = [a[name]["rerank_ms"] for a in out["alternations"]]
        out[name + "_rerank_ms"] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=0, help="rows of the corpus (default: C3's 10 M)")
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dot_c3_bench.json"))
    args = ap.parse_args()
    import torch
    import bench
    import pq_vector_amd as pqv
    n, dim, kc, nprobe, _ = bench.WORKLOADS["c3"]
    if args.rows:
        n = args.rows
    k = 10
    dev = torch.device("cuda", 0)
    corpus_t = bench.synth(torch, dev, 1234, n, dim)
    q_t = bench.synth(torch, dev, 7, 64, dim)
    torch.cuda.synchronize()
    corpus = pqv.Corpus.from_device_ptr(corpus_t.data_ptr(), n, dim, device=0, keepalive=corpus_t)
    t0 = time.perf_counter()
    index = pqv.IndexBuilder(corpus).n_clusters(kc).max_iters(20).seed(42).workers(min(16, os.cpu_count() or 1)).build()
    build_s = time.perf_counter() - t0
    s = pqv.Searcher(index, corpus)
    s.set_option("rerank_mode", 1)                                       # the L2 baseline: stream_kernel, as DOT's twin
    s.set_timing(True)
    st = torch.cuda.Stream()
    rec = {"workload": "c3", "rows": n, "dim": dim, "n_clusters": kc, "nprobe": nprobe, "k": k, "index_build_s": build_s,
           "describe_dot": s.describe(64, k, nprobe, pqv.PQV_DOT), "describe_l2_stream": s.describe(64, k, nprobe)}
    rec["one_query"] = shape(torch, pqv, s, st, q_t[:1], k, nprobe, dim, args.alternations, args.calls)
    rec["batch_64"] = shape(torch, pqv, s, st, q_t, k, nprobe, dim, args.alternations, args.calls)
    # every list probed: the same rows for both metrics (fewer calls: a 64-query call streams the whole corpus 64 times)
    few = max(1, args.calls // 5)
    rec["all_lists_one_query"] = shape(torch, pqv, s, st, q_t[:1], k, kc, dim, args.alternations, few)
    rec["all_lists_batch_64"] = shape(torch, pqv, s, st, q_t, k, kc, dim, args.alternations, few)
    log(json.dumps({x: {y: rec[x][y] for y in ("dot_over_l2_call", "dot_over_l2_rerank", "dot_rerank_ms", "l2_stream_rerank_ms")}
                    for x in ("one_query", "batch_64", "all_lists_one_query", "all_lists_batch_64")}))
    s.close(); corpus.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({x: rec[x] for x in ("rows", "describe_dot")})[:1500])


if __name__ == "__main__":
    main()
