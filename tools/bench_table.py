#!/usr/bin/env python3
"""A table of indexed files on one GPU (TableSearcher) against the per-file route and one ordinary index.

Rows and queries are bench.py's C3 synth (10 M x 768 uniform, seed 1234; queries seed 7).  Two tables over the same rows:
  t8  -- 8 files of 1.25 M rows, 128 clusters each, nprobe 4 per file (P = 32 lists per query, as C3)
  t64 -- 64 files of 156 250 rows, 16 clusters each, nprobe 1 per file (P = 64)
and for each, on the same queries (1024-query batches and single queries):
  (a) table   -- one TableSearcher, one pqv_topk_device call
  (b) perfile -- one Searcher per file, one pqv_topk_device call each, the per-file lists copied out and merged on the host
                 (pqv_merge_topk); the time includes that copy and merge
  (c) single  -- one ordinary index over all rows (C3's 1024 clusters) with the same P (nprobe 32 / 64)
k = 10, sqrt_out = 0.  Reported per route: queries/s (host clock around synchronised calls, median of --reps), the fraction
bytes-over-HBM-peak computed as bench.py's roofline does (the int8 image of every distinct probed row + 8 bytes, plus the f32
row of every screen survivor) over the CALL time, and whether (a) and (b) agree.  Kernel times: run this under
`rocprofv3 --kernel-trace --stats` in a run of its own.  Prints one JSON line.
--max-candidates M[,M...] adds the capped leg per shape and M (VectorTopKOptions::max_candidates, dealt out round robin
over the files as the reference's CandidateCursor does):
  (a) capped   -- a TableSearcher created with PQV_TABLE_CAP_ROUND_ROBIN, one pqv_topk_device call
  (b) perfile  -- the route without it: per query, the per-file candidate counts (pqv_probe + list lengths), the quotas
                  (pqv_round_robin_quota), one capped pqv_topk_device call per (query, file), pqv_merge_topk; timed on the first
                  --cap-subset queries of a batch and scaled to the batch
  (c) uncapped -- the uncapped table at the same nprobe
usage: python tools/bench_table.py [--reps N] [--shapes t8,t64] [--max-candidates 2048,32768] [--cap-subset 16] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K = 10


def timed(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="t8,t64")
    ap.add_argument("--out", default="")
    ap.add_argument("--max-candidates", default="")
    ap.add_argument("--cap-subset", type=int, default=16)
    args = ap.parse_args()
    import torch
    import bench
    import pq_vector_amd as pqv
    n, dim, kc, _, nq = bench.WORKLOADS["c3"]
    dev = torch.device("cuda", 0)
    corpus_t = bench.synth(torch, dev, 1234, n, dim)
    q_t = bench.synth(torch, dev, 7, nq, dim)
    torch.cuda.synchronize()
    workers = min(16, os.cpu_count() or 1)
    corpus = pqv.Corpus.from_device_ptr(corpus_t.data_ptr(), n, dim, device=0, keepalive=corpus_t)
    t0 = time.perf_counter()
    single_index = pqv.IndexBuilder(corpus).n_clusters(kc).max_iters(20).seed(42).workers(workers).build()
    single = pqv.Searcher(single_index, corpus)
    single_lens = np.diff(np.asarray(single_index.list_offsets, dtype=np.int64))
    out = {"rows": n, "dim": dim, "k": K, "batch": nq, "single_index_build_s": time.perf_counter() - t0, "shapes": {}}

    def run(s, queries, k, nprobe, max_candidates=0):
        m = len(queries)
        rows = torch.empty((m, k), dtype=torch.int32, device=dev)
        dist = torch.empty((m, k), dtype=torch.float32, device=dev)
        nf = torch.empty(m, dtype=torch.int32, device=dev)
        s.topk_device(queries.data_ptr(), m, k, nprobe, rows.data_ptr(), dist.data_ptr(), nf.data_ptr(), 0,
                      max_candidates=max_candidates, sqrt_out=False)
        return rows, dist, nf

    def roofline(s, queries, nprobe, sec, probe_lists):
        """bench.py's min_bytes over the call time: int8 image + 8 B of every distinct probed row, f32 row of every survivor."""
        c0 = s.counters()
        run(s, queries, K, nprobe)
        torch.cuda.synchronize()
        surv = s.counters()["screen_survivors"] - c0["screen_survivors"]
        distinct = probe_lists(queries)
        plan = s.describe(len(queries), K, nprobe)
        opb = 1 if "int8 screen operands" in plan else 2 if "f16 screen operands" in plan else 4
        mb = distinct * (opb * dim + 8) + surv * 4 * dim
        return {"min_bytes": int(mb), "frac_of_peak_over_call": mb / sec / 1e9 / bench.HBM_PEAK_GBS, "plan": plan}

    for shape in [x for x in args.shapes.split(",") if x]:
        F, kc_f, nprobe_f = {"t8": (8, 128, 4), "t64": (64, 16, 1)}[shape]
        per = n // F
        row_base = [f * per for f in range(F)]
        t0 = time.perf_counter()
        idx, files = [], []
        for f in range(F):
            sl = corpus_t[row_base[f]:row_base[f] + per]
            c_f = pqv.Corpus.from_device_ptr(sl.data_ptr(), per, dim, device=0, keepalive=sl)
            idx.append(pqv.IndexBuilder(c_f).n_clusters(kc_f).max_iters(20).seed(42).workers(workers).build())
            files.append(c_f)
        build_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        table = pqv.TableSearcher(idx, corpus, row_base)
        table_create_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        perfile = [pqv.Searcher(ix, c_f) for ix, c_f in zip(idx, files)]
        perfile_create_s = time.perf_counter() - t0
        P = table.probe_count(nprobe_f)
        lens_t = np.concatenate([np.diff(np.asarray(ix.list_offsets, dtype=np.int64)) for ix in idx])
        rec = {"files": F, "clusters_per_file": kc_f, "nprobe_per_file": nprobe_f, "P": P, "index_builds_s": build_s,
               "table_create_s": table_create_s, "perfile_create_s": perfile_create_s, "by_nq": {}}

        def perfile_call(queries, k=K):
            outs = [run(s_f, queries, k, nprobe_f) for s_f in perfile]
            torch.cuda.synchronize()            # (each searcher runs on its own stream: the copies below must follow all of them)
            r = np.stack([o[0].cpu().numpy().view(np.uint32) for o in outs])
            r = np.where(r == 0xFFFFFFFF, r, r.astype(np.int64) + np.asarray(row_base, np.int64)[:, None, None]).astype(np.uint32)
            d = np.stack([o[1].cpu().numpy() for o in outs])
            c = np.stack([o[2].cpu().numpy().astype(np.uint32) for o in outs])
            return pqv.merge_topk(d, r, c)

        def probed_table(queries):
            ids = set(x for q in queries.cpu().numpy() for x in table.probe(q, nprobe_f).tolist())
            return int(lens_t[sorted(ids)].sum())

        def probed_single(queries):
            ids = set(x for q in queries.cpu().numpy() for x in single.probe(q, P).tolist())
            return int(single_lens[sorted(ids)].sum())

        for m in (nq, 1):
            qb = q_t[:m].contiguous()
            ta = timed(torch, lambda: run(table, qb, K, nprobe_f), args.reps)
            tb = timed(torch, lambda: perfile_call(qb), args.reps)
            tc = timed(torch, lambda: run(single, qb, K, P), args.reps)
            ra, da, fa = run(table, qb, K, nprobe_f)
            torch.cuda.synchronize()
            md, mr, _, mc = perfile_call(qb)
            same = bool((fa.cpu().numpy().astype(np.uint32) == mc).all() and
                        (ra.cpu().numpy().view(np.uint32) == mr).all() and
                        (da.cpu().numpy().view(np.uint32) == md.view(np.uint32)).all())
            r = {"table": {"s": ta, "qps": m / ta}, "perfile": {"s": tb, "qps": m / tb}, "single_index": {"s": tc, "qps": m / tc},
                 "table_equals_perfile_merge": same, "table_over_single": tc / ta, "table_over_perfile": tb / ta}
            if m == nq:
                r["table"].update(roofline(table, qb, nprobe_f, ta, probed_table))
                r["single_index"].update(roofline(single, qb, P, tc, probed_single))
            rec["by_nq"][str(m)] = r
        rec["describe_table_1024"] = table.describe(nq, K, nprobe_f)
        rec["describe_table_1"] = table.describe(1, K, nprobe_f)
        caps = [int(x) for x in args.max_candidates.split(",") if x]
        if caps:
            capped = pqv.TableSearcher(idx, corpus, row_base, pqv.PQV_TABLE_CAP_ROUND_ROBIN)
            lens_f = [np.diff(np.asarray(ix.list_offsets, dtype=np.int64)) for ix in idx]

            def perfile_capped(queries, mc):
                """(b): rows u32 [m, K], dist [m, K], counts [m] -- per query and file one capped call, then the merge"""
                qs = queries.cpu().numpy()
                rows_o, dist_o, cnt_o = [], [], []
                for i, q in enumerate(qs):
                    counts = np.array([int(lens_f[f][s_f.probe(q, nprobe_f)].sum()) for f, s_f in enumerate(perfile)], np.uint64)
                    quota = pqv.round_robin_quota(counts, mc)
                    outs = [(f, run(s_f, queries[i:i + 1], K, nprobe_f, int(quota[f]))) for f, s_f in enumerate(perfile) if quota[f]]
                    torch.cuda.synchronize()
                    r = np.full((F, 1, K), 0xFFFFFFFF, np.uint32)
                    d = np.full((F, 1, K), np.inf, np.float32)
                    c = np.zeros((F, 1), np.uint32)
                    for f, o in outs:
                        rf = o[0].cpu().numpy().view(np.uint32)
                        r[f] = np.where(rf == 0xFFFFFFFF, rf, rf.astype(np.int64) + row_base[f]).astype(np.uint32)
                        d[f] = o[1].cpu().numpy()
                        c[f] = o[2].cpu().numpy().astype(np.uint32)
                    md, mr, _, mcnt = pqv.merge_topk(d, r, c)
                    rows_o.append(mr[0]); dist_o.append(md[0]); cnt_o.append(mcnt[0])
                return np.stack(rows_o), np.stack(dist_o), np.array(cnt_o)

            rec["capped"] = {}
            for mc in caps:
                by = {}
                for m in (nq, 1):
                    qb = q_t[:m].contiguous()
                    sub = qb[:min(m, args.cap_subset)].contiguous()
                    ta = timed(torch, lambda: run(capped, qb, K, nprobe_f, mc), args.reps)
                    tb_sub = timed(torch, lambda: perfile_capped(sub, mc), max(1, args.reps // 2))
                    tb = tb_sub * m / len(sub)
                    tc = timed(torch, lambda: run(table, qb, K, nprobe_f), args.reps)
                    ra, da, fa = run(capped, sub, K, nprobe_f, mc)
                    torch.cuda.synchronize()
                    br, bd, bc = perfile_capped(sub, mc)
                    same = bool((fa.cpu().numpy().astype(np.uint32) == bc).all() and (ra.cpu().numpy().view(np.uint32) == br).all() and
                                (da.cpu().numpy().view(np.uint32) == bd.view(np.uint32)).all())
                    by[str(m)] = {"capped": {"s": ta, "qps": m / ta}, "perfile_capped": {"s": tb, "qps": m / tb, "timed_queries": len(sub)},
                                  "uncapped": {"s": tc, "qps": m / tc}, "capped_equals_perfile": same,
                                  "capped_over_uncapped_time": ta / tc, "perfile_over_capped_time": tb / ta}
                rec["capped"][str(mc)] = by
            rec["describe_capped_1024"] = capped.describe(nq, K, nprobe_f)
            del capped
        out["shapes"][shape] = rec
        del table, perfile
        torch.cuda.synchronize()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
