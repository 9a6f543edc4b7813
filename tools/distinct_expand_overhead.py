#!/usr/bin/env python3
"""What "probe on until k GROUPS are found" costs next to the two fixed-depth distinct calls it replaces.

1 M x 128 uniform rows (bench.py's synth, seed 1234), 1024 lists, a group column of 4 rows per group (a random assignment, so a
group's rows lie in different lists), a random 1/SEL row mask (--sels, default 64,1024: one index, one result line per mask), 1024
queries per call (seed 7), k = 10 (--k).
Device forms, warmed; the variants ALTERNATE in one process, each call between two device events on one stream:
  (a) pqv_topk_distinct_device at nprobe 8    (b) pqv_topk_distinct_expand_device 8 -> 64    (c) pqv_topk_distinct_device at nprobe 64
  (r) pqv_topk_expand_device 8 -> 64 under the same mask: the ROW-counting expansion, whose filter_count_kernel +
      expand_select_kernel are the yardstick of group_expand_kernel in a kernel trace (--only b,r)
Prints one JSON line per mask: median ms per call of each, the mean and max nprobe_used of (b), the share of queries with
n_found == k in (a), (b) and (c), and the embeddings each variant fetched per call.
usage: python tools/distinct_expand_overhead.py [--reps 50] [--sels 64,1024] [--k 10] [--only a,b,c,r] [--max-iters 5]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--only", default="a,b,c")
    ap.add_argument("--max-iters", type=int, default=5)
    ap.add_argument("--sels", default="64,1024", help="each mask allows one row in SEL")
    ap.add_argument("--k", type=int, default=10)
    args = ap.parse_args()
    import torch
    import bench
    import pq_vector_amd as pqv
    n, dim, kc, nq, k, lo, hi = 1_000_000, 128, 1024, 1024, args.k, 8, 64
    dev = torch.device("cuda", 0)
    corpus_t = bench.synth(torch, dev, 1234, n, dim)
    q_t = bench.synth(torch, dev, 7, nq, dim)
    torch.cuda.synchronize()
    corpus = pqv.Corpus.from_device_ptr(corpus_t.data_ptr(), n, dim, device=0, keepalive=corpus_t)
    index = pqv.IndexBuilder(corpus).n_clusters(kc).max_iters(args.max_iters).seed(42).workers(min(16, os.cpu_count() or 1)).build()
    s = pqv.Searcher(index, corpus)
    rng = np.random.default_rng(99)
    doc = (rng.permutation(n) // 4).astype(np.int64)
    col = pqv.Column.upload(doc, None, device=0)
    keys = s.row_keys(col)
    col.close()
    r_t = torch.empty((nq, k), dtype=torch.int32, device=dev)
    d_t = torch.empty((nq, k), dtype=torch.float32, device=dev)
    g_t = torch.empty((nq, k), dtype=torch.int64, device=dev)
    nf_t = torch.zeros(nq, dtype=torch.int32, device=dev)
    nc_t = torch.zeros(nq, dtype=torch.int64, device=dev)
    u_t = torch.zeros(nq, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream()
    hs = stream.cuda_stream
    names = args.only.split(",")
    for sel in (int(x) for x in args.sels.split(",")):
        mask = s.row_mask(rng.random(n) < 1 / sel)

        def call(nprobe, max_nprobe=0):
            s.topk_distinct_device(q_t.data_ptr(), nq, k, nprobe, keys, r_t.data_ptr(), d_t.data_ptr(), g_t.data_ptr(), nf_t.data_ptr(),
                                   nc_t.data_ptr(), sqrt_out=False, mask=mask, stream=hs, max_nprobe=max_nprobe,
                                   d_nprobe_used=u_t.data_ptr() if max_nprobe else 0)

        def rows_call():
            s.topk_device(q_t.data_ptr(), nq, k, lo, r_t.data_ptr(), d_t.data_ptr(), nf_t.data_ptr(), nc_t.data_ptr(), sqrt_out=False,
                          mask=mask, stream=hs, max_nprobe=hi, d_nprobe_used=u_t.data_ptr())

        variants = {"a": lambda: call(lo), "b": lambda: call(lo, hi), "c": lambda: call(hi), "r": rows_call}
        out = {"rows": n, "dim": dim, "lists": kc, "queries": nq, "k": k, "rows_per_group": 4, "mask": f"1/{sel}", "nprobe": lo,
               "max_nprobe": hi, "reps": args.reps}
        for v in names:          # warm-up, and what each variant answers
            variants[v]()
            stream.synchronize()
            before = s.counters()["embeddings_fetched"]
            variants[v]()
            stream.synchronize()
            out[f"{v}_full_share"] = float((nf_t == k).float().mean().item())
            out[f"{v}_embeddings_per_call"] = int(s.counters()["embeddings_fetched"] - before)
            if v in ("b", "r"):
                out[f"{v}_mean_nprobe_used"] = float(u_t.float().mean().item())
                out[f"{v}_max_nprobe_used"] = int(u_t.max().item())
        stream.synchronize()
        times = {v: [] for v in names}
        with torch.cuda.stream(stream):
            for _ in range(args.reps):
                for v in names:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    variants[v]()
                    e1.record(stream)
                    times[v].append((e0, e1))
        stream.synchronize()
        for v in names:
            ms = sorted(a.elapsed_time(b) for a, b in times[v])
            out[f"{v}_ms"] = round(ms[len(ms) // 2], 4)
            out[f"{v}_ms_min_max"] = [round(ms[0], 4), round(ms[-1], 4)]
        print(json.dumps(out), flush=True)
        mask.close()
    keys.close()
    s.close()


if __name__ == "__main__":
    main()
