#!/usr/bin/env python3
"""What one batched distinct call with a filter PER QUERY costs next to what a caller had to do without it.

1 M x 128 uniform rows (bench.py's synth, seed 1234), 1024 lists, a tenant column of T tenants (--tenants, default 16; 256 is the
other documented point) and a doc column of about 16 chunks per doc (both from seed 99), 1024 queries per call (seed 7), query q of
tenant q % T, k = 10, nprobe 8.  Device forms, warmed, each timed between two device events on one stream; the variants alternate:
  (n) pqv_topk_distinct_filtered_device, one call, the tenants as a device-resident PQV_KEY_EQ filter
  (a) 1024 single-query pqv_topk_distinct_device calls, each under the prebuilt row mask of its tenant (the masks are built before
      the clock starts; their construction is timed separately, per mask)
  (b) pqv_topk_distinct_device of the same batch without any filter: the floor on work
Prints one JSON line: median ms per batch of each, the embeddings each variant fetched per batch, the ms one mask takes to build,
and whether (n) and (a) returned the same rows.
usage: python tools/distinct_filter_overhead.py [--reps 20] [--tenants 16] [--max-iters 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--tenants", type=int, default=16)
    ap.add_argument("--max-iters", type=int, default=5)
    args = ap.parse_args()
    import torch
    import bench
    import pq_vector_amd as pqv
    n, dim, kc, nq, k, nprobe, T = 1_000_000, 128, 1024, 1024, 10, 8, args.tenants
    dev = torch.device("cuda", 0)
    corpus_t = bench.synth(torch, dev, 1234, n, dim)
    q_t = bench.synth(torch, dev, 7, nq, dim)
    torch.cuda.synchronize()
    corpus = pqv.Corpus.from_device_ptr(corpus_t.data_ptr(), n, dim, device=0, keepalive=corpus_t)
    index = pqv.IndexBuilder(corpus).n_clusters(kc).max_iters(args.max_iters).seed(42).workers(min(16, os.cpu_count() or 1)).build()
    s = pqv.Searcher(index, corpus)
    rng = np.random.default_rng(99)
    tenant = rng.integers(0, T, n).astype(np.int32)
    doc = rng.integers(0, n // 16, n).astype(np.int64)
    keys = {}
    for name, v in (("tenant", tenant), ("doc", doc)):
        col = pqv.Column.upload(v, None, device=0)
        keys[name] = s.row_keys(col)
        col.close()
    qkeys = (np.arange(nq) % T).astype(np.int64)
    qk_t = torch.from_numpy(qkeys).to(dev)
    # (a)'s masks: one per tenant, built before the clock starts; what building one costs is reported on its own
    t0 = time.perf_counter()
    masks = [s.row_mask(tenant == t) for t in range(T)]
    mask_ms = (time.perf_counter() - t0) * 1e3 / T
    r_t = torch.empty((nq, k), dtype=torch.int32, device=dev)
    d_t = torch.empty((nq, k), dtype=torch.float32, device=dev)
    g_t = torch.empty((nq, k), dtype=torch.int64, device=dev)
    nf_t = torch.zeros(nq, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream()
    hs = stream.cuda_stream
    qp, rp, dp, gp, fp = q_t.data_ptr(), r_t.data_ptr(), d_t.data_ptr(), g_t.data_ptr(), nf_t.data_ptr()

    def new():
        s.topk_distinct_device(qp, nq, k, nprobe, keys["doc"], rp, dp, gp, fp, sqrt_out=False, stream=hs, filter_keys=keys["tenant"],
                               query_keys=qk_t.data_ptr())

    def singles():
        for q in range(nq):
            s.topk_distinct_device(qp + q * dim * 4, 1, k, nprobe, keys["doc"], rp + q * k * 4, dp + q * k * 4, gp + q * k * 8, fp + q * 4,
                                   sqrt_out=False, stream=hs, mask=masks[q % T])

    def floor():
        s.topk_distinct_device(qp, nq, k, nprobe, keys["doc"], rp, dp, gp, fp, sqrt_out=False, stream=hs)

    variants = {"n": new, "a": singles, "b": floor}
    out = {"rows": n, "dim": dim, "lists": kc, "queries": nq, "k": k, "nprobe": nprobe, "tenants": T, "reps": args.reps,
           "mask_build_ms_per_mask": round(mask_ms, 3), "masks_built": T}
    rows_of = {}
    for v in variants:          # warm-up, and what each variant fetches
        variants[v]()
        stream.synchronize()
        before = s.counters()["embeddings_fetched"]
        variants[v]()
        stream.synchronize()
        out[f"{v}_embeddings_per_batch"] = int(s.counters()["embeddings_fetched"] - before)
        out[f"{v}_full_share"] = float((nf_t == k).float().mean().item())
        rows_of[v] = r_t.cpu().numpy().copy()
    out["n_equals_a"] = bool((rows_of["n"] == rows_of["a"]).all())
    times = {v: [] for v in variants}
    with torch.cuda.stream(stream):
        for _ in range(args.reps):
            for v in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                variants[v]()
                e1.record(stream)
                times[v].append((e0, e1))
    stream.synchronize()
    for v in variants:
        ms = sorted(a.elapsed_time(b) for a, b in times[v])
        out[f"{v}_ms"] = round(ms[len(ms) // 2], 4)
        out[f"{v}_ms_min_max"] = [round(ms[0], 4), round(ms[-1], 4)]
    print(json.dumps(out))
    for m in masks:
        m.close()
    for kk in keys.values():
        kk.close()
    s.close()


if __name__ == "__main__":
    main()
