#!/usr/bin/env python3
"""Distinct top-k against the two existing routes next to it (bench.py's synth: uniform rows, seed 1234; 1 M x 128; 100 clusters;
nprobe 8; k 10; 64-query batches, queries seed 7; group column int64, every key value on `g` rows, g in {1, 16, 256}).

On ONE searcher, in the same run, per group size:
  distinct  ONE pqv_topk_distinct_device call;
  (a)       pqv_topk_masked_device under an all-ones row mask: the same streaming pass and fold without groups (k chunks, not k
            documents -- the cost floor of the pass);
  (b)       the only exact route without this entry point: pqv_range_search_masked with radius = +inf (every considered row of every
            query sorted and copied to the host) and the first row per key kept with numpy.
The three alternate rep by rep.  Times are host clock from the call to the end of a device synchronisation (route (b) to the end of
the host pass), medians of --reps after one warm-up.  Writes one JSON line (profiles/distinct_bench.json is that line).
usage: python tools/bench_distinct.py [--rows N] [--reps N]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

K, NQ, DIM, KC, NPROBE, GROUP_ROWS = 10, 64, 128, 100, 8, (1, 16, 256)


def stats(times):
    ms = np.asarray(times) * 1e3
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max())}


def group_column(n, g):
    """every key value on g rows, scattered over the corpus; values beyond 32 bits"""
    return (np.random.default_rng(3000 + g).permutation(n) // g).astype(np.int64) * (2 ** 32 + 3) - 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import torch
    import bench
    import distinct_ref
    import pq_vector_amd as pqv
    dev = torch.device("cuda", 0)
    n = args.rows
    corpus_t = bench.synth(torch, dev, 1234, n, DIM)
    q_t = bench.synth(torch, dev, 7, NQ, DIM)
    torch.cuda.synchronize()
    q_h = q_t.cpu().numpy()
    corpus = pqv.Corpus.from_device_ptr(corpus_t.data_ptr(), n, DIM, device=0, keepalive=corpus_t)
    index = pqv.IndexBuilder(corpus).n_clusters(KC).max_iters(5).seed(42).workers(min(16, os.cpu_count() or 1)).build()
    s = pqv.Searcher(index, corpus)
    rows = torch.zeros((NQ, K), dtype=torch.int32, device=dev)
    dist = torch.zeros((NQ, K), dtype=torch.float32, device=dev)
    grp = torch.zeros((NQ, K), dtype=torch.int64, device=dev)
    nf = torch.zeros(NQ, dtype=torch.int32, device=dev)
    ones = s.row_mask(np.ones(n, bool))
    out = {"rows": n, "dim": DIM, "clusters": KC, "nprobe": NPROBE, "k": K, "nq": NQ, "reps": args.reps, "groups": []}

    def timed(call):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for g in GROUP_ROWS:
        values = group_column(n, g)
        col = pqv.Column.upload(values)
        keys = s.row_keys(col)
        col.close()
        host_result = {}

        def distinct():
            s.topk_distinct_device(q_t.data_ptr(), NQ, K, NPROBE, keys, rows.data_ptr(), dist.data_ptr(), grp.data_ptr(), nf.data_ptr(),
                                   sqrt_out=False)

        def masked():
            s.topk_device(q_t.data_ptr(), NQ, K, NPROBE, rows.data_ptr(), dist.data_ptr(), sqrt_out=False, mask=ones)

        def range_dedup():
            lims, r, d, _, _ = s.range_search(q_h, np.inf, NPROBE, sqrt_out=False, mask=ones)
            host_result["rows"] = [distinct_ref.dedup_sorted(r[int(lims[i]):int(lims[i + 1])], d[int(lims[i]):int(lims[i + 1])], values, K)[0]
                                   for i in range(NQ)]

        calls = (("distinct", distinct), ("masked_all_ones", masked), ("range_inf_host_dedup", range_dedup))
        for _, c in calls:
            timed(c)
        t = {name: [] for name, _ in calls}
        for _ in range(args.reps):
            for name, c in calls:
                t[name].append(timed(c))
        distinct()
        torch.cuda.synchronize()
        got = rows.cpu().numpy().view(np.uint32)
        same = all((got[i, :len(e)] == e).all() for i, e in enumerate(host_result["rows"]))
        r = {"rows_per_key": g, **{name: stats(v) for name, v in t.items()}, "routes_agree": bool(same),
             "distinct_over_masked": float(np.median(t["distinct"]) / np.median(t["masked_all_ones"])),
             "range_dedup_over_distinct": float(np.median(t["range_inf_host_dedup"]) / np.median(t["distinct"]))}
        out["groups"].append(r)
        print(json.dumps(r), file=sys.stderr, flush=True)
        keys.close()
    ones.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
