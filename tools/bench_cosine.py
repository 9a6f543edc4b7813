#!/usr/bin/env python3
"""PQV_COSINE through the index (include/pqv.h: PQV_COSINE), measured; writes profiles/cosine_bench.json.

  c3   bench.py's C3 (10 M x 768 uniform, seed 1234; 1024 clusters; nprobe 32; k 10; queries seed 7): pqv_topk_device queries/s
       at 1024-query steps, cosine against L2 on the same searcher; single-query p50 (host clock around a synchronised
       pqv_topk_device call) for both; kernel launches per call from the counters; the time of the first cosine call (the layout
       is built there) and the footprint before / after it.
  c5   10 M x 1536 (bench.synth_mixture with ceil(sqrt(n)) centres: embedding-like clustered rows -- on uniform rows no IVF probe
       of 32 lists finds the true neighbours), the default cluster count, nprobe 32, k 10:
       cosine through the index against pqv_brute_topk(PQV_COSINE) -- queries/s of both at 1024 queries, recall@10 of the
       index against the brute-force result.
  --trace   runs `rocprofv3 --kernel-trace --stats` over `--part c3 --steps 5 --single 50` in a child process of its own and
            adds the per-kernel summary (tools/rocpd_summary.py) to the record.
usage: python tools/bench_cosine.py [--part c3|c5|all] [--steps N] [--single N] [--trace] [--out PATH]"""
import argparse
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def log(*a):
    print(*a, file=sys.stderr, flush=True)


_STREAM = []


def _stream(torch):
    """One explicit stream for every timed call (handle 0 would name the searcher's own stream, not torch's default one)."""
    if not _STREAM:
        torch.cuda.synchronize()
        _STREAM.append(torch.cuda.Stream())
    return _STREAM[0]


def batch_qps(torch, s, q_t, k, nprobe, metric, steps, warmup=3):
    nq = q_t.shape[0]
    dev = q_t.device
    r_t = torch.empty((nq, k), dtype=torch.int32, device=dev)
    d_t = torch.empty((nq, k), dtype=torch.float32, device=dev)
    st = _stream(torch)
    for _ in range(warmup):
        s.topk_device(q_t.data_ptr(), nq, k, nprobe, r_t.data_ptr(), d_t.data_ptr(), metric=metric, sqrt_out=False, stream=st.cuda_stream)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(steps):
        s.topk_device(q_t.data_ptr(), nq, k, nprobe, r_t.data_ptr(), d_t.data_ptr(), metric=metric, sqrt_out=False, stream=st.cuda_stream)
    e1.record(st)
    st.synchronize()
    ms = e0.elapsed_time(e1) / steps
    return {"ms_per_step": ms, "q_per_s": nq / (ms / 1e3)}


def single_p50(torch, s, q_t, k, nprobe, metric, n):
    dev = q_t.device
    r_t = torch.empty((1, k), dtype=torch.int32, device=dev)
    d_t = torch.empty((1, k), dtype=torch.float32, device=dev)
    st = _stream(torch)
    c0 = s.counters()["kernel_launches"]
    times = []
    for i in range(n + 5):
        q = q_t[i % q_t.shape[0]:i % q_t.shape[0] + 1]
        st.synchronize()
        t0 = time.perf_counter()
        s.topk_device(q.data_ptr(), 1, k, nprobe, r_t.data_ptr(), d_t.data_ptr(), metric=metric, sqrt_out=False, stream=st.cuda_stream)
        st.synchronize()
        if i >= 5:
            times.append(time.perf_counter() - t0)
    launches = (s.counters()["kernel_launches"] - c0) / (n + 5)
    return {"p50_us": float(np.median(times) * 1e6), "p99_us": float(np.percentile(times, 99) * 1e6), "calls": n,
            "counted_launches_per_call": launches}


def part_c3(pqv, torch, args):
    import bench
    n, dim, kc, nprobe, nq = bench.WORKLOADS["c3"]
    k = 10
    dev = torch.device("cuda", 0)
    corpus_t = bench.synth(torch, dev, 1234, n, dim)
    q_t = bench.synth(torch, dev, 7, nq, dim)
    torch.cuda.synchronize()
    corpus = pqv.Corpus.from_device_ptr(corpus_t.data_ptr(), n, dim, device=0, keepalive=corpus_t)
    t0 = time.perf_counter()
    index = pqv.IndexBuilder(corpus).n_clusters(kc).max_iters(20).seed(42).workers(os.cpu_count() or 1).build()
    build_s = time.perf_counter() - t0
    s = pqv.Searcher(index, corpus)
    out = {"workload": "c3", "rows": n, "dim": dim, "n_clusters": kc, "nprobe": nprobe, "k": k, "batch": nq, "index_build_s": build_s}
    out["footprint_before"] = s.footprint()
    out["l2_batch"] = batch_qps(torch, s, q_t, k, nprobe, pqv.PQV_L2SQ_REF4, args.steps)
    out["l2_single"] = single_p50(torch, s, q_t, k, nprobe, pqv.PQV_L2SQ_REF4, args.single)
    # the first cosine call builds the layout: its wall time less a later call's is the preparation
    q1 = q_t[:1]
    r_t = torch.empty((1, k), dtype=torch.int32, device=dev)
    d_t = torch.empty((1, k), dtype=torch.float32, device=dev)
    st = _stream(torch)
    st.synchronize()
    t0 = time.perf_counter()
    s.topk_device(q1.data_ptr(), 1, k, nprobe, r_t.data_ptr(), d_t.data_ptr(), metric=pqv.PQV_COSINE, stream=st.cuda_stream)
    st.synchronize()
    first_s = time.perf_counter() - t0
    out["footprint_after"] = s.footprint()
    out["cosine_batch"] = batch_qps(torch, s, q_t, k, nprobe, pqv.PQV_COSINE, args.steps)
    out["cosine_single"] = single_p50(torch, s, q_t, k, nprobe, pqv.PQV_COSINE, args.single)
    out["prepare_s"] = first_s - out["cosine_single"]["p50_us"] / 1e6
    fb, fa = out["footprint_before"], out["footprint_after"]
    out["footprint_added_bytes"] = fa["total_bytes"] - fb["total_bytes"]
    out["column_bytes"] = n * dim * 4
    out["cosine_over_l2_batch_time"] = out["cosine_batch"]["ms_per_step"] / out["l2_batch"]["ms_per_step"]
    out["describe_l2"] = s.describe(nq, k, nprobe)
    out["describe_cosine"] = s.describe(nq, k, nprobe, pqv.PQV_COSINE)
    out["describe_cosine_single"] = s.describe(1, k, nprobe, pqv.PQV_COSINE)
    log(json.dumps({x: out[x] for x in ("l2_batch", "cosine_batch", "l2_single", "cosine_single", "prepare_s")}))
    s.close(); corpus.close()
    del corpus_t
    return out


def part_c5(pqv, torch, args):
    import bench
    n, dim = bench.WORKLOADS["c5"][:2]
    nq, k, nprobe = 1024, 10, 32
    dev = torch.device("cuda", 0)
    kc = int(np.ceil(np.sqrt(n)))                                # the default cluster count (index.rs:161-167)
    corpus_t = bench.synth_mixture(torch, dev, 1234, n, dim, kc)
    q_t = bench.synth_mixture(torch, dev, 7, nq, dim, kc)
    torch.cuda.synchronize()
    corpus = pqv.Corpus.from_device_ptr(corpus_t.data_ptr(), n, dim, device=0, keepalive=corpus_t)
    t0 = time.perf_counter()
    index = pqv.IndexBuilder(corpus).max_iters(20).seed(42).workers(os.cpu_count() or 1).build()
    build_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    s = pqv.Searcher(index, corpus, pqv.PQV_PREPARE_COSINE)
    create_s = time.perf_counter() - t0
    out = {"workload": "c5", "rows": n, "dim": dim, "n_clusters": index.n_clusters, "nprobe": nprobe, "k": k, "batch": nq,
           "index_build_s": build_s, "searcher_create_with_prepare_s": create_s, "footprint": s.footprint()}
    out["cosine_batch"] = batch_qps(torch, s, q_t, k, nprobe, pqv.PQV_COSINE, args.steps)
    out["l2_batch"] = batch_qps(torch, s, q_t, k, nprobe, pqv.PQV_L2SQ_REF4, args.steps)
    qs = q_t.cpu().numpy()
    rows, dist, nf, _ = s.topk(qs, k, nprobe, metric=pqv.PQV_COSINE)
    corpus.brute_topk(qs[:8], k, pqv.PQV_COSINE)                  # warm-up: the brute screen's images are built here
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        brows, bdist, bnf = corpus.brute_topk(qs, k, pqv.PQV_COSINE)
        times.append(time.perf_counter() - t0)
    bt = float(np.median(times))
    out["brute_batch"] = {"s_per_call": bt, "q_per_s": nq / bt}
    hits = [len(set(rows[i, :nf[i]].tolist()) & set(brows[i, :bnf[i]].tolist())) for i in range(nq)]
    out["recall_at_10_vs_brute"] = float(np.mean(hits) / k)
    out["cosine_index_over_brute_qps"] = out["cosine_batch"]["q_per_s"] / out["brute_batch"]["q_per_s"]
    out["describe_cosine"] = s.describe(nq, k, nprobe, pqv.PQV_COSINE)
    log(json.dumps({x: out[x] for x in ("cosine_batch", "brute_batch", "recall_at_10_vs_brute")}))
    s.close(); corpus.close()
    del corpus_t
    return out


def trace():
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--part", "c3",
               "--steps", "5", "--single", "50", "--out", os.path.join(d, "child.json")]
        log("trace:", " ".join(cmd))
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=900)
        dbs = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)
        lines = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "rocpd_summary.py"), dbs[0], "--match", "pqv"],
                               check=True, capture_output=True, text=True).stdout.splitlines()
    return {"command": "rocprofv3 --kernel-trace --stats -- python tools/bench_cosine.py --part c3 --steps 5 --single 50",
            "summary": [l for l in lines if l.strip() and " summary of " not in l][:40]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=["c3", "c5", "all"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--single", type=int, default=200)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cosine_bench.json"))
    args = ap.parse_args()
    rec = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            rec = json.load(f)
    if args.trace:
        rec["kernel_trace_c3"] = trace()
    else:
        import torch
        import pq_vector_amd as pqv
        if args.part in ("c3", "all"):
            rec["c3"] = part_c3(pqv, torch, args)
        if args.part in ("c5", "all"):
            rec["c5"] = part_c5(pqv, torch, args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: v for k, v in rec.items() if k != "kernel_trace_c3"})[:2000])


if __name__ == "__main__":
    main()
