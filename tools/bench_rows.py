#!/usr/bin/env python3
"""Candidate lists against key partitions over the SAME row sets (bench.py's synth: uniform rows, seed 1234; 2^20 rows of 128 and of
768 dims; 1024 queries, seed 7; k 10; device entry points).

The rows are dealt to tenants of exactly C rows each (C in {256, 4096}; a random deal, seed 1000 + C), every query asks for one
tenant (seed 2000 + C), and
  (a) ONE pqv_topk_rows_device call gets the tenant's rows as the query's candidate list, ascending;
  (b) ONE pqv_topk_partition_device call with PQV_KEY_EQ gets the tenant's key: the same rows in the same order from the partition.
Both read 4 dim bytes per candidate; (a) adds two gathered words per candidate (the row id, then its list position from the row
map) where (b) reads one (the partition's list position, contiguous).  The index is 1024 lists dealt at random (no k-means: only
the list order matters here, and a random one is what a row id's list position looks like), the searcher has the default layout.
Both alternate inside one timed loop.  Times are host clock from the enqueue to the end of a device synchronisation, medians with
minimum and maximum of --reps after two warm-ups of each; the outputs of the two calls are compared (they must be equal bit for
bit: pqv.h).  Writes one JSON line (profiles/rows_bench.json holds it).
usage: python tools/bench_rows.py [--reps N] [--dims 128,768]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, KC, K, NQ, PER_QUERY = 1 << 20, 1024, 10, 1024, (256, 4096)


def stats(times):
    ms = np.asarray(times) * 1e3
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--dims", default="128,768")
    args = ap.parse_args()
    import torch
    import bench
    import pq_vector_amd as pqv
    dev = torch.device("cuda", 0)
    out = {"rows": N, "n_clusters": KC, "k": K, "nq": NQ, "reps": args.reps, "cases": []}
    for dim in [int(x) for x in args.dims.split(",")]:
        corpus_t = bench.synth(torch, dev, 1234, N, dim)
        q_t = bench.synth(torch, dev, 7, NQ, dim)
        torch.cuda.synchronize()
        corpus = pqv.Corpus.from_device_ptr(corpus_t.data_ptr(), N, dim, device=0, keepalive=corpus_t)
        deal = np.random.default_rng(99).permutation(N).astype(np.uint32)
        index = pqv.Index.from_parts(dim, np.zeros((KC, dim), np.float32), [np.sort(deal[i::KC]) for i in range(KC)])
        s = pqv.Searcher(index, corpus)

        def outputs():
            return (torch.zeros((NQ, K), dtype=torch.int32, device=dev), torch.zeros((NQ, K), dtype=torch.float32, device=dev),
                    torch.zeros(NQ, dtype=torch.int32, device=dev), torch.zeros(NQ, dtype=torch.int64, device=dev))

        def timed_once(enqueue):
            t0 = time.perf_counter()
            enqueue()
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        for c in PER_QUERY:
            tenant = np.empty(N, np.int32)
            tenant[np.random.default_rng(1000 + c).permutation(N)] = np.arange(N, dtype=np.int32) // c
            qkeys = np.random.default_rng(2000 + c).integers(0, N // c, NQ).astype(np.int64)
            by_tenant = np.argsort(tenant, kind="stable").astype(np.uint32).reshape(N // c, c)      # a tenant's rows, ascending
            cand = np.ascontiguousarray(by_tenant[qkeys]).reshape(-1)
            lims = np.arange(NQ + 1, dtype=np.int64) * c
            col = pqv.Column.upload(tenant)
            part = s.key_partition(col)
            col.close()
            qk_t = torch.from_numpy(qkeys).to(dev)
            lims_t = torch.from_numpy(lims).to(dev)
            cand_t = torch.from_numpy(cand.view(np.int32)).to(dev)
            ro, pa = outputs(), outputs()

            def rows_call():
                s.topk_rows_device(q_t.data_ptr(), NQ, K, lims_t.data_ptr(), cand_t.data_ptr(), ro[0].data_ptr(), ro[1].data_ptr(),
                                   ro[2].data_ptr(), ro[3].data_ptr())

            def partition_call():
                s.topk_partition_device(q_t.data_ptr(), NQ, K, part, pa[0].data_ptr(), pa[1].data_ptr(), pa[2].data_ptr(), pa[3].data_ptr(),
                                        query_keys=qk_t.data_ptr())

            for _ in range(2):
                timed_once(rows_call)
                timed_once(partition_call)
            c0 = s.counters()
            timed_once(rows_call)
            c1 = s.counters()
            t_a, t_b = [], []
            for _ in range(args.reps):
                t_a.append(timed_once(rows_call))
                t_b.append(timed_once(partition_call))
            same = all(bool((x == y).all()) for x, y in zip((t.cpu().numpy() for t in ro), (t.cpu().numpy() for t in pa)))
            considered = int(c1["embeddings_fetched"] - c0["embeddings_fetched"])
            cands = int(c1["candidate_rows"] - c0["candidate_rows"])
            r = {"dim": dim, "candidates_per_query": c, "outputs_equal": same, "considered_rows": considered, "candidate_rows": cands,
                 "rows": {**stats(t_a), "bytes": float(considered * 4 * dim + cands * 8)},
                 "partition": {**stats(t_b), "bytes": float(considered * 4 * dim + cands * 4)},
                 "rows_over_partition": float(np.median(t_a) / np.median(t_b))}
            out["cases"].append(r)
            print(json.dumps(r), file=sys.stderr, flush=True)
            part.close()
        s.close()
        index.close()
        corpus.close()
        del corpus_t, q_t
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
