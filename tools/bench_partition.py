#!/usr/bin/env python3
"""Key partitions against today's only batched route to a per-tenant answer (bench.py's synth: uniform rows, seed 1234; 1024
clusters; k 10; 1024 queries, seed 7; device entry points; I32 keys uniform over T tenants, T in {16, 1024, 65536}; every query
asks for one tenant's rows).

  (a) ONE pqv_topk_partition_device call with PQV_KEY_EQ: exact, nothing probed.
  (b) ONE pqv_topk_expand_device call with PQV_KEY_EQ, nprobe = 32 and max_nprobe = n_clusters: approximate -- a query stops
      probing once k passing rows are in its lists.
Both alternate inside one timed loop.  Times are host clock from the enqueue to the end of a device synchronisation, medians with
minimum and maximum of --reps after one warm-up of each.  Beside the times: the share of queries where (b) finds fewer than k rows
or other rows than (a), and each side's bytes per call, computed from what the kernels read --
  (a) considered rows x 4 dim (the embeddings_fetched counter) + candidate positions x 4 (the partition's list positions);
  (b) considered rows x 4 dim + the key column of every list the counting pass and the stream pass walk: the counting pass all
      P = max_nprobe = n_clusters lists (n positions per query), the stream pass the used ones (n_candidates[q] positions), x 4.
--mask FRACTION runs (a) under a shared row mask that allows that fraction of the rows (uniform, seed 3000): the masked walk of
partition_stream_kernel.  (b) stays unmasked, so the comparisons between the sides mean nothing then; the line carries "mask".
Writes one JSON line (profiles/partition_bench.json holds those lines).
usage: python tools/bench_partition.py [--workload c3s|c3] [--reps N] [--mask FRACTION]"""
import argparse
import json
import os
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c3s", choices=["c3s", "c3"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--mask", type=float, default=None, metavar="FRACTION")
    args = ap.parse_args()
    import torch
    import bench
    import pq_vector_amd as pqv
    n, dim, kc, nprobe, _ = bench.WORKLOADS[args.workload]
    dev = torch.device("cuda", 0)
    corpus_t = bench.synth(torch, dev, 1234, n, dim)
    q_t = bench.synth(torch, dev, 7, NQ, dim)
    torch.cuda.synchronize()
    corpus = pqv.Corpus.from_device_ptr(corpus_t.data_ptr(), n, dim, device=0, keepalive=corpus_t)
    index = pqv.IndexBuilder(corpus).n_clusters(kc).max_iters(20).seed(42).workers(min(16, os.cpu_count() or 1)).build()
    s = pqv.Searcher(index, corpus)
    list_len = np.diff(index.list_offsets.astype(np.int64))
    mask = s.row_mask(np.random.default_rng(3000).random(n) < args.mask) if args.mask is not None else None

    def outputs():
        return (torch.zeros((NQ, K), dtype=torch.int32, device=dev), torch.zeros((NQ, K), dtype=torch.float32, device=dev),
                torch.zeros(NQ, dtype=torch.int32, device=dev), torch.zeros(NQ, dtype=torch.int64, device=dev))

    def timed_once(enqueue):
        t0 = time.perf_counter()
        enqueue()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    out = {"workload": args.workload, "rows": n, "dim": dim, "n_clusters": kc, "nprobe": nprobe, "max_nprobe": kc, "k": K, "nq": NQ,
           "reps": args.reps, "tenants": []}
    if mask is not None:
        out["mask"] = args.mask
    for t in TENANTS:
        col = pqv.Column.upload(tenant_column(n, t))
        t0 = time.perf_counter()
        part = s.key_partition(col)
        part_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        keys = s.row_keys(col)
        keys_ms = (time.perf_counter() - t0) * 1e3
        col.close()
        qk_t = torch.from_numpy(query_keys(NQ, t)).to(dev)
        pa, ex = outputs(), outputs()
        used_t = torch.zeros(NQ, dtype=torch.int32, device=dev)

        def partition_call():
            s.topk_partition_device(q_t.data_ptr(), NQ, K, part, pa[0].data_ptr(), pa[1].data_ptr(), pa[2].data_ptr(), pa[3].data_ptr(),
                                    query_keys=qk_t.data_ptr(), mask=mask)

        def expand_call():
            s.topk_device(q_t.data_ptr(), NQ, K, nprobe, ex[0].data_ptr(), ex[1].data_ptr(), ex[2].data_ptr(), ex[3].data_ptr(),
                          keys=keys, query_keys=qk_t.data_ptr(), max_nprobe=kc, d_nprobe_used=used_t.data_ptr())

        timed_once(partition_call)
        timed_once(expand_call)
        c0 = s.counters()
        timed_once(partition_call)
        c1 = s.counters()
        timed_once(expand_call)
        c2 = s.counters()
        t_a, t_b = [], []
        for _ in range(args.reps):
            t_a.append(timed_once(partition_call))
            t_b.append(timed_once(expand_call))
        a_rows, a_found = pa[0].cpu().numpy(), pa[2].cpu().numpy()
        b_rows, b_found = ex[0].cpu().numpy(), ex[2].cpu().numpy()
        used = used_t.cpu().numpy().astype(np.int64)
        short = b_found < np.minimum(K, a_found)
        differ = short | (a_rows != b_rows).any(axis=1)
        a_considered = c1["embeddings_fetched"] - c0["embeddings_fetched"]
        b_considered = c2["embeddings_fetched"] - c1["embeddings_fetched"]
        # (b)'s key bytes: the counting pass reads the key column of all P = kc lists per query (every position once), the stream pass
        # that of the lists the query used -- n_candidates[q] is their summed length
        b_key_bytes = float((NQ * int(list_len.sum()) + int(ex[3].cpu().numpy().astype(np.int64).sum())) * 4)
        r = {"tenants": t, "rows_per_tenant": n / t, "partition_create_ms": part_ms, "row_keys_create_ms": keys_ms,
             "partition": {**stats(t_a), "considered_rows": int(a_considered), "candidate_rows": int(c1["candidate_rows"] - c0["candidate_rows"]),
                           "bytes": float(a_considered * 4 * dim + (c1["candidate_rows"] - c0["candidate_rows"]) * 4)},
             "expand": {**stats(t_b), "considered_rows": int(b_considered), "mean_nprobe_used": float(used.mean()),
                        "bytes": float(b_considered * 4 * dim + b_key_bytes)},
             "expand_over_partition": float(np.median(t_b) / np.median(t_a)),
             "expand_queries_short_of_k": float(short.mean()), "expand_queries_with_other_rows": float(differ.mean())}
        out["tenants"].append(r)
        print(json.dumps(r), file=sys.stderr, flush=True)
        part.close()
        keys.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
