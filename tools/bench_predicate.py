#!/usr/bin/env python3
"""Time to a usable row mask, 10 M rows: the routes that take allow bytes or a host-evaluated expression against predicates
evaluated on the GPU over resident columns (pqv_row_mask_from_predicates).

The cost of a mask depends on n_rows and the id table only, so the corpus is 10 M x 8 zeros and the index 1024 hand-made lists
(Index.from_parts) over a random permutation of the rows.  Columns: id (int32, = row), price (float64, 10 % NULL), ts (int64,
10 % NULL), qty (float32).  Every route produces the mask of the same kind of predicate and is timed from the call to the
returned, complete mask (creation synchronises its stream before it returns), after --warmup rounds, over --reps rounds in which
the routes ALTERNATE; medians and min / max are reported.

  (a) bytes_host        Searcher.row_mask(bool array): n bytes over PCIe, mask_layout_kernel + mask_pack_kernel
      bytes_device      Searcher.row_mask_device(device bytes): the n-byte host copy back, the same kernels
      expression_file   parquet_io.row_mask_from_expression(file, pc.field("id") >= n / 2) + Searcher.row_mask: what
                        .where(pyarrow expression) does per query
  (b) pred_i32          id >= n / 2
      pred_mixed3       (id >= n / 4) & (qty < 0.5) | (ts between a, b)
      pred_i64_f64      (ts >= a) & (price < 0.25)          -- both columns with validity bytes

Least bytes per kernel (what it must move: DESIGN 5.15) are always reported; with --kernel-stats FILE (the kernel stats CSV of a
separate `rocprofv3 --kernel-trace --stats -- python tools/bench_predicate.py --profile-run all` run) each kernel's average time
and its least bytes / time as a share of the HBM peak are added.  --profile-run creates masks five times per route and measures
nothing itself: `all` the three predicates and the byte-made mask, `predicates` the three predicates only (for a
`rocprofv3 --memory-copy-trace` run: after the set-up's uploads every copy is the 8-byte allowed total).  Writes profiles/predicate_bench.json (--out) and prints the same JSON line.
usage: python tools/bench_predicate.py [--rows N] [--reps R] [--warmup W] [--kernel-stats FILE] [--profile-run all|predicates] [--out PATH]"""
import argparse
import csv
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12


def setup(pqv, torch, n):
    dev = torch.device("cuda", 0)
    rows_t = torch.zeros((n, 8), dtype=torch.float32, device=dev)
    corpus = pqv.Corpus.from_device_ptr(rows_t.data_ptr(), n, 8, device=0, keepalive=rows_t)
    rng = np.random.default_rng(1)
    perm = rng.permutation(n).astype(np.uint32)
    lists = np.array_split(perm, 1024)
    s = pqv.Searcher(pqv.Index.from_parts(8, rng.random((1024, 8), dtype=np.float32), lists), corpus)
    cols = {"id": (np.arange(n, dtype=np.int32), None),
            "price": (rng.random(n), (rng.random(n) >= 0.1).astype(np.uint8)),
            "ts": (rng.integers(0, 1 << 40, n).astype(np.int64), (rng.random(n) >= 0.1).astype(np.uint8)),
            "qty": (rng.random(n, dtype=np.float32), None)}
    for name, (values, valid) in cols.items():
        s.attach_column(name, pqv.Column.upload(values, valid))
    return s, cols, rows_t


def predicates(pqv, n):
    c = pqv.col
    return {"pred_i32": (c("id") >= n // 2, ["id"]),
            "pred_mixed3": (((c("id") >= n // 4) & (c("qty") < 0.5)) | c("ts").between(1 << 38, 1 << 39), ["id", "qty", "ts"]),
            "pred_i64_f64": ((c("ts") >= (1 << 39)) & (c("price") < 0.25), ["ts", "price"])}


def least_bytes(cols, names, n, n_pos):
    rows = sum(n * (cols[x][0].dtype.itemsize + (0 if cols[x][1] is None else 1)) for x in names) + n // 8
    return {"predicate_rows_kernel": rows, "mask_gather_kernel": n_pos * 4 + n_pos // 8 + n // 8}


def kernel_stats(path):
    """{kernel name (up to the first parenthesis): average ns} from a rocprofv3 kernel stats CSV"""
    out = {}
    for row in csv.DictReader(open(path)):
        name = (row.get("Name") or row.get("KernelName") or "").split("(")[0].split("::")[-1]
        avg = row.get("AverageNs") or row.get("Average") or row.get("AverageDurationNs")
        if name and avg:
            out[name] = float(avg)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-stats")
    ap.add_argument("--profile-run", choices=["all", "predicates"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predicate_bench.json"))
    args = ap.parse_args()
    import torch
    import pq_vector_amd as pqv
    from pq_vector_amd import parquet_io
    n = args.rows
    s, cols, _keep = setup(pqv, torch, n)
    preds = predicates(pqv, n)
    allowed = np.arange(n) >= n // 2
    allowed_t = torch.from_numpy(allowed).to(torch.device("cuda", 0))
    torch.cuda.synchronize()

    if args.profile_run:
        for _ in range(5):
            for p, _names in preds.values():
                s.row_mask(p).close()
            if args.profile_run == "all":
                s.row_mask(allowed).close()
        return

    import pyarrow as pa
    import pyarrow.compute as pc
    import pyarrow.parquet as pq
    tmp = tempfile.mkdtemp(prefix="pqv_predicate_bench_")
    path = os.path.join(tmp, "scalars.parquet")
    pq.write_table(pa.table({"id": pa.array(cols["id"][0])}), path)
    expr = pc.field("id") >= n // 2

    routes = {"bytes_host": lambda: s.row_mask(allowed),
              "bytes_device": lambda: s.row_mask_device(allowed_t.data_ptr(), n),
              "expression_file": lambda: s.row_mask(parquet_io.row_mask_from_expression(path, expr))}
    for name, (p, _names) in preds.items():
        routes[name] = (lambda p=p: s.row_mask(p))
    times = {name: [] for name in routes}
    counts = {}
    for rep in range(args.warmup + args.reps):
        for name, make in routes.items():
            t0 = time.perf_counter()
            m = make()
            dt = time.perf_counter() - t0
            counts[name] = m.count
            m.close()
            if rep >= args.warmup:
                times[name].append(dt)
    assert counts["bytes_host"] == counts["bytes_device"] == counts["expression_file"] == counts["pred_i32"] == n - n // 2
    out = {"rows": n, "lists": 1024, "reps": args.reps, "warmup": args.warmup, "hbm_peak_TBps": HBM_PEAK / 1e12, "routes": {}, "kernels": {}}
    for name, ts in times.items():
        out["routes"][name] = {"ms_median": float(np.median(ts) * 1e3), "ms_min": float(np.min(ts) * 1e3), "ms_max": float(np.max(ts) * 1e3),
                               "allowed": int(counts[name]), "group": "b" if name.startswith("pred_") else "a"}
    stats = kernel_stats(args.kernel_stats) if args.kernel_stats else {}
    for name, (_p, names) in preds.items():
        out["kernels"][name] = least_bytes(cols, names, n, n)
    out["kernels"]["bytes"] = {"mask_pack_kernel": n + n // 8, "mask_layout_kernel": n * 4 + n + n // 8}
    if stats:
        # one stats file averages a kernel over every route of the profile run: the predicate kernel's bytes are the routes' mean
        mean_rows = float(np.mean([out["kernels"][x]["predicate_rows_kernel"] for x in preds]))
        least = {"predicate_rows_kernel": mean_rows, "mask_gather_kernel": out["kernels"]["pred_i32"]["mask_gather_kernel"],
                 "mask_pack_kernel": out["kernels"]["bytes"]["mask_pack_kernel"], "mask_layout_kernel": out["kernels"]["bytes"]["mask_layout_kernel"]}
        out["kernel_times"] = {k: {"avg_us": stats[k] / 1e3, "least_bytes": b, "share_of_hbm_peak": b / (stats[k] * 1e-9) / HBM_PEAK}
                               for k, b in least.items() if k in stats}
    else:
        out["kernel_times"] = "not measured"
    os.remove(path)
    os.rmdir(tmp)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
