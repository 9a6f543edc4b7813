#!/usr/bin/env python3
"""Row-masked top-k on C3 (bench.py's synth: 10 M x 768 uniform, seed 1234; 1024 clusters; nprobe 32; k 10; queries seed 7).

Masks: random at selectivity 1, 1/2, 1/8, 1/64, 1/1024, and the contiguous predicate row >= n / 2.  For nq = 1 and nq = 64 under
each mask, after a warm-up and over --reps repetitions: call time (host clock around the synchronous call), the re-rank pass
(masked_stream_kernel) from pqv_set_timing, the considered rows (the embeddings_fetched counter) x 4 dim bytes over that time
and their fraction of 8 TB/s.
Baseline (a): the unmasked call with rerank_mode = 1 (stream_kernel, the same exact pass without a mask) on the same searcher,
alternating with the masked all-ones call -- ratio of the medians and the spread of the repetitions.
Baseline (b): today's only route to the masked answer -- unmasked pqv_topk with k raised (doubling) until k allowed rows survive
the host filter -- timed on a few queries and scaled to the batch.
Prints one JSON line.
usage: python tools/bench_masked.py [--reps N] [--baseline-queries M] [--no-baseline]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(s, call, reps):
    """-> (call seconds per repetition, re-rank ms per call, device span ms per call)"""
    call()
    s.timing_read()
    s.set_timing(True)
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
    s.set_timing(False)
    rr_ms, total_ms, _ = s.timing_read()
    return times, rr_ms / reps, total_ms / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-queries", type=int, default=4)
    ap.add_argument("--no-baseline", action="store_true")
    args = ap.parse_args()
    import torch
    import bench
    import pq_vector_amd as pqv
    n, dim, kc, nprobe, _ = bench.WORKLOADS["c3"]
    k = 10
    dev = torch.device("cuda", 0)
    corpus_t = bench.synth(torch, dev, 1234, n, dim)
    queries = bench.synth(torch, dev, 7, 64, dim).cpu().numpy()
    torch.cuda.synchronize()
    corpus = pqv.Corpus.from_device_ptr(corpus_t.data_ptr(), n, dim, device=0, keepalive=corpus_t)
    index = pqv.IndexBuilder(corpus).n_clusters(kc).max_iters(20).seed(42).workers(os.cpu_count() or 1).build()
    s = pqv.Searcher(index, corpus)
    rng = np.random.default_rng(99)
    masks = {"all": np.ones(n, bool)}
    for d in (2, 8, 64, 1024):
        masks[f"random_1/{d}"] = rng.random(n) < 1.0 / d
    masks["row>=n/2"] = np.arange(n) >= n // 2
    out = {"workload": "c3", "rows": n, "dim": dim, "n_clusters": kc, "nprobe": nprobe, "k": k, "reps": args.reps,
           "hbm_peak_TBps": 8.0, "configs": []}
    for name, allowed in masks.items():
        t0 = time.perf_counter()
        m = s.row_mask(allowed)
        create_s = time.perf_counter() - t0
        for nq in (1, 64):
            qs = queries[:nq]
            c0 = s.counters()
            s.topk(qs, k, nprobe, mask=m)
            c1 = s.counters()
            considered = c1["embeddings_fetched"] - c0["embeddings_fetched"]
            candidates = c1["candidate_rows"] - c0["candidate_rows"]
            times, rr_ms, span_ms = timed(s, lambda: s.topk(qs, k, nprobe, mask=m), args.reps)
            bytes_ = considered * 4 * dim
            cfg = {"mask": name, "allowed_rows": m.count, "mask_create_ms": create_s * 1e3, "nq": nq,
                   "candidates": int(candidates), "considered_rows": int(considered), "expected_f32_bytes": int(bytes_),
                   "call_ms_median": float(np.median(times) * 1e3), "call_ms_min": float(np.min(times) * 1e3),
                   "call_ms_max": float(np.max(times) * 1e3), "rerank_ms": rr_ms, "device_span_ms": span_ms,
                   "rerank_TBps": bytes_ / (rr_ms / 1e3) / 1e12 if rr_ms else None,
                   "rerank_frac_of_8TBps": bytes_ / (rr_ms / 1e3) / 8e12 if rr_ms else None}
            out["configs"].append(cfg)
            print(json.dumps(cfg), file=sys.stderr, flush=True)
        if name == "all":
            # baseline (a): the unmasked exact stream (rerank_mode = 1) alternating with the masked all-ones call
            out["baseline_unmasked_stream"] = []
            for nq in (1, 64):
                qs = queries[:nq]
                t_m, t_u, rr_m, rr_u = [], [], [], []
                for _ in range(args.reps):
                    tm, rm, _ = timed(s, lambda: s.topk(qs, k, nprobe, mask=m), 1)
                    s.set_option("rerank_mode", 1)
                    tu, ru, _ = timed(s, lambda: s.topk(qs, k, nprobe), 1)
                    s.set_option("rerank_mode", 0)
                    t_m += tm; t_u += tu; rr_m.append(rm); rr_u.append(ru)
                b = {"nq": nq, "masked_call_ms": [x * 1e3 for x in t_m], "unmasked_call_ms": [x * 1e3 for x in t_u],
                     "masked_rerank_ms": rr_m, "unmasked_rerank_ms": rr_u,
                     "rerank_ratio_of_medians": float(np.median(rr_m) / np.median(rr_u)),
                     "rerank_spread": {"masked": [float(np.min(rr_m)), float(np.max(rr_m))],
                                       "unmasked": [float(np.min(rr_u)), float(np.max(rr_u))]}}
                out["baseline_unmasked_stream"].append(b)
                print(json.dumps(b), file=sys.stderr, flush=True)
        if not args.no_baseline and name != "all":
            # baseline (b): over-fetch with a larger k and filter on the host, k doubled until k allowed rows survive
            per_q, ks = [], []
            for i in range(min(args.baseline_queries, len(queries))):
                t0 = time.perf_counter()
                kk = 4 * k
                while True:
                    rows, dist, nf, nc = s.topk(queries[i:i + 1], kk, nprobe)
                    r = rows[0, :nf[0]]
                    keep = r[allowed[r]]
                    if len(keep) >= k or nf[0] < kk or kk >= int(nc[0]):
                        break
                    kk *= 2
                per_q.append(time.perf_counter() - t0)
                ks.append(kk)
            masked_64 = [c for c in out["configs"] if c["mask"] == name and c["nq"] == 64][0]["call_ms_median"] / 1e3
            out.setdefault("baseline_overfetch", []).append(
                {"mask": name, "queries_timed": len(per_q), "final_k": ks, "s_per_query": float(np.mean(per_q)),
                 "s_for_64_scaled": float(np.mean(per_q)) * 64, "masked_64_s": masked_64,
                 "speedup_at_64": float(np.mean(per_q)) * 64 / masked_64})
            print(json.dumps(out["baseline_overfetch"][-1]), file=sys.stderr, flush=True)
        m.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
