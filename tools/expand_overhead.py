#!/usr/bin/env python3
"""What "probe on until k rows pass" costs next to the two fixed-depth calls it replaces.

1 M x 128 uniform rows (bench.py's synth, seed 1234), 1024 lists, a random 1/SEL row mask (--sel, default 64), 1024 queries per
call (seed 7), k = 10 (--k).
Device form, warmed; the three variants ALTERNATE in one process, each call between two device events on one stream:
  (a) pqv_topk_masked_device at nprobe 8      (b) pqv_topk_expand_device 8 -> 64      (c) pqv_topk_masked_device at nprobe 64
Prints one JSON line: median ms per call of each, the mean nprobe_used of (b), the share of queries with n_found == k in (a),
(b) and (c), and the embeddings each variant fetched per call.
--only b --reps N: just the expanding call, for a kernel trace of its count and select launches.
usage: python tools/expand_overhead.py [--reps 50] [--sel 64] [--k 10] [--only a|b|c] [--max-iters 5]"""
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
    ap.add_argument("--only", choices=("a", "b", "c"))
    ap.add_argument("--max-iters", type=int, default=5)
    ap.add_argument("--sel", type=int, default=64, help="the mask allows one row in SEL")
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
    allowed = np.random.default_rng(99).random(n) < 1 / args.sel
    mask = s.row_mask(allowed)
    r_t = torch.empty((nq, k), dtype=torch.int32, device=dev)
    d_t = torch.empty((nq, k), dtype=torch.float32, device=dev)
    nf_t = torch.zeros(nq, dtype=torch.int32, device=dev)
    nc_t = torch.zeros(nq, dtype=torch.int64, device=dev)
    u_t = torch.zeros(nq, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream()
    hs = stream.cuda_stream

    def call(nprobe, max_nprobe=0):
        s.topk_device(q_t.data_ptr(), nq, k, nprobe, r_t.data_ptr(), d_t.data_ptr(), nf_t.data_ptr(), nc_t.data_ptr(), sqrt_out=False,
                      mask=mask, stream=hs, max_nprobe=max_nprobe, d_nprobe_used=u_t.data_ptr() if max_nprobe else 0)

    variants = {"a": lambda: call(lo), "b": lambda: call(lo, hi), "c": lambda: call(hi)}
    names = [args.only] if args.only else ["a", "b", "c"]
    out = {"rows": n, "dim": dim, "lists": kc, "queries": nq, "k": k, "mask": f"1/{args.sel}", "nprobe": lo, "max_nprobe": hi, "reps": args.reps}
    for v in names:          # warm-up, and what each variant answers
        variants[v]()
        stream.synchronize()
        before = s.counters()["embeddings_fetched"]
        variants[v]()
        stream.synchronize()
        out[f"{v}_full_share"] = float((nf_t == k).float().mean().item())
        out[f"{v}_embeddings_per_call"] = int(s.counters()["embeddings_fetched"] - before)
        if v == "b":
            out["b_mean_nprobe_used"] = float(u_t.float().mean().item())
            out["b_max_nprobe_used"] = int(u_t.max().item())
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
    print(json.dumps(out))
    mask.close()
    s.close()


if __name__ == "__main__":
    main()
