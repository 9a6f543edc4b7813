#!/usr/bin/env python3
"""What per-query probe depths cost and buy (pqv.h: pqv_topk_depth).  Two corpora -- 1 M x 128 uniform, the shape of
5.19's table, and bench.py's Gaussian mixture (sigma 0.1, one component per list) -- 1024 queries, k = 10, device form, device
events on one explicit stream, the variants alternating in one process:

  a   the uniform call at nprobe = p0 = 8                c   the uniform call at nprobe = P = 64
  g   GIVEN, every depth 8, max_nprobe = 64              r   RATIO at a few ratios (nprobe 1, max_nprobe 64)

g walks what a walks and ranks what c ranks.  The cost condition: t(g) < (t(a) + t(c)) / 2 -- ranks nobody walks cost nothing
beyond ranking P centroids.  For r: mean / max nprobe_used and recall@10 against brute_topk, beside a and c (reported, not gated).
Writes profiles/depth_bench.json."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--mixture-rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--p0", type=int, default=8)
    ap.add_argument("--P", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--recall-queries", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_bench.json"))
    args = ap.parse_args()

    import torch
    import bench
    import pq_vector_amd as pqv

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream()
    nq, k, p0, P = args.nq, args.k, args.p0, args.P
    result = {"nq": nq, "k": k, "p0": p0, "P": P, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "shapes": {}}

    shapes = [("uniform", args.rows, 0, (1.01, 1.02, 1.04, 1.08)), ("mixture", args.mixture_rows, 1024, (1.5, 2.0, 3.0, 5.0))]
    for name, n, kc, ratios in shapes:
        if name == "uniform":
            corpus_t, q_t = bench.synth(torch, dev, 1234, n, args.dim), bench.synth(torch, dev, 7, nq, args.dim)
        else:
            corpus_t, q_t = bench.synth_mixture(torch, dev, 1234, n, args.dim, kc), bench.synth_mixture(torch, dev, 7, nq, args.dim, kc)
        torch.cuda.synchronize()
        corpus = pqv.Corpus.from_device_ptr(corpus_t.data_ptr(), n, args.dim, device=0, keepalive=corpus_t)
        b = pqv.IndexBuilder(corpus).max_iters(20).seed(42).workers(min(16, os.cpu_count() or 1))
        index = b.n_clusters(kc).build() if kc else b.build()
        srch = pqv.Searcher(index, corpus)
        rows_t = torch.zeros((nq, k), dtype=torch.int32, device=dev)
        dist_t = torch.zeros((nq, k), dtype=torch.float32, device=dev)
        nf_t = torch.zeros(nq, dtype=torch.int32, device=dev)
        nc_t = torch.zeros(nq, dtype=torch.int64, device=dev)
        used_t = torch.zeros(nq, dtype=torch.int32, device=dev)
        eights = torch.full((nq,), p0, dtype=torch.int32, device=dev)

        def call(nprobe, **kw):
            srch.topk_device(q_t.data_ptr(), nq, k, nprobe, rows_t.data_ptr(), dist_t.data_ptr(), nf_t.data_ptr(), nc_t.data_ptr(),
                             stream=stream.cuda_stream, **kw)

        variants = {"a": lambda: call(p0), "c": lambda: call(P),
                    "g": lambda: call(p0, max_nprobe=P, probe_depths=eights.data_ptr(), d_nprobe_used=used_t.data_ptr())}
        for r in ratios:
            variants[f"r{r}"] = (lambda r=r: call(1, max_nprobe=P, d2_ratio=r, d_nprobe_used=used_t.data_ptr()))
        times = {v: [] for v in variants}
        with torch.cuda.stream(stream):
            for it in range(args.warmup + args.rounds):
                for v, fn in variants.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    fn()
                    e1.record(stream)
                    e1.synchronize()
                    if it >= args.warmup:
                        times[v].append(e0.elapsed_time(e1))
        m = min(args.recall_queries, nq)
        q_host = q_t[:m].cpu().numpy()
        truth, _, _ = corpus.brute_topk(q_host, k, pqv.PQV_L2SQ_MFMA)
        rec = {"rows": n, "dim": args.dim, "n_clusters": index.n_clusters, "plan_at_P": srch.describe(nq, k, P), "variants": {}}
        for v, fn in variants.items():
            with torch.cuda.stream(stream):
                used_t.fill_(p0 if v == "a" else P)
                fn()
            stream.synchronize()
            got = rows_t[:m].cpu().numpy().view(np.uint32)
            used = used_t.cpu().numpy()
            t = np.array(times[v])
            rec["variants"][v] = {"ms_median": float(np.median(t)), "ms_min": float(t.min()), "ms_p90": float(np.percentile(t, 90)),
                                  "nprobe_used_mean": float(used.mean()), "nprobe_used_max": int(used.max()),
                                  "recall_at_k": sum(len(set(got[i].tolist()) & set(truth[i].tolist())) for i in range(m)) / float(m * k)}
        ta, tc, tg = (rec["variants"][v]["ms_median"] for v in "acg")
        rec["cost_condition"] = {"t_a_ms": ta, "t_c_ms": tc, "t_g_ms": tg, "midpoint_ms": (ta + tc) / 2, "holds": bool(tg < (ta + tc) / 2)}
        result["shapes"][name] = rec
        print(name, json.dumps(rec["cost_condition"]), flush=True)
        for v, x in rec["variants"].items():
            print(f"  {v:6s} {x['ms_median']:.3f} ms  used mean {x['nprobe_used_mean']:.2f} max {x['nprobe_used_max']}  recall@{k} {x['recall_at_k']:.4f}", flush=True)
        srch.close(); corpus.close()
        del corpus_t
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0 if all(s["cost_condition"]["holds"] for s in result["shapes"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
