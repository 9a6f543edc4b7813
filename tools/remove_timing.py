#!/usr/bin/env python3
"""Times index remove and compact on one GPU, in one process: at a given shape (default C2's: 1 M x 128, 100
clusters), with a random `--fraction` of the rows removed,
  1. pqv_index_remove_device (flags resident on the GPU) against the only other route to that index without k-means:
     Index.from_parts(empty lists).append(corpus of the surviving rows) -- a route made of calls older than remove, so it runs
     the same on the commit before it --, the upload of the surviving rows timed apart;
  2. list_compact_kernel between HIP events beside a device-to-device copy of the same list bytes (the library's
     PQV_REMOVE_STATS=1 line, switched on for these calls only);
  3. pqv_index_compact against uploading the surviving rows from the host and indexing them with with_centroids;
  4. rows_gather_kernel between HIP events beside a device-to-device copy of the same row bytes;
  5. with --search: one --nq query batch at k 10 on the removed index, unmasked, against the same batch on the old searcher under
     the equivalent mask, with the describe string of each.
Five repetitions after a warm-up, median [min, max].  Prints one JSON line; --out also appends it to a file (one line per shape).  The removed and the
compacted index are compared with their definitions in numpy first, so a wrong result cannot be timed."""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn, reps):
    out, ts = None, []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, ts


def _mmm(ts):
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)} if ts else None


def _stats_lines(fn, reps, prefix):
    """Runs fn() `reps` times with PQV_REMOVE_STATS=1 and the process' stderr in a file; -> the library's lines."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        os.environ["PQV_REMOVE_STATS"] = "1"
        try:
            for _ in range(reps):
                fn()
        finally:
            del os.environ["PQV_REMOVE_STATS"]
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        return [l for l in f.read().decode().splitlines() if l.startswith(prefix)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--clusters", type=int, default=100)
    ap.add_argument("--fraction", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--search", action="store_true")
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, default=8)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import pq_vector_amd as pqv

    rng = np.random.default_rng(2)
    X = rng.random((a.rows, a.dim), dtype=np.float32)
    flags = rng.random(a.rows) < a.fraction
    keep = np.nonzero(~flags)[0]
    corpus = pqv.Corpus.upload(X)
    index = pqv.IndexBuilder(corpus).n_clusters(a.clusters).build()
    d_flags = torch.from_numpy(flags).to(torch.device("cuda", 0))
    torch.cuda.synchronize()

    # 1, 2: remove
    remove = lambda: index.remove(flags=d_flags)                                  # noqa: E731
    remove()                                                                      # warm-up: code objects, pools
    removed, t_remove = _timed(remove, a.reps)
    off, rows = index.list_offsets.astype(np.int64), index.list_rows
    want = [rows[off[c]:off[c + 1]] for c in range(a.clusters)]
    want = [l[~flags[l]] for l in want]
    assert np.array_equal(removed.list_rows, np.concatenate(want)) and removed.row_bound == a.rows
    assert np.array_equal(removed.list_offsets, np.concatenate([[0], np.cumsum([len(l) for l in want])]))
    lines_r = _stats_lines(remove, a.reps, "pqv_index_remove:")
    pat = re.compile(r"compaction kernel ([0-9.]+) ms for ([0-9]+) list bytes .* copy of the same bytes ([0-9.]+) ms")
    got = [g for g in (pat.search(l) for l in lines_r) if g]
    t_kernel, t_lcopy = [float(g.group(1)) for g in got], [float(g.group(3)) for g in got]
    list_bytes = int(got[0].group(2)) if got else 0

    # the other route: the surviving rows as a corpus of their own, indexed under the same centroids
    Xs = np.ascontiguousarray(X[keep])
    survivors, t_upload = _timed(lambda: pqv.Corpus.upload(Xs), 1)
    empty = pqv.Index.from_parts(a.dim, index.centroids, [np.zeros(0, np.uint32)] * a.clusters)
    empty.append(survivors)
    _, t_route = _timed(lambda: empty.append(survivors), a.reps)

    # 3, 4: compact
    compact = lambda: removed.compact(corpus)                                     # noqa: E731
    compact()
    (dense, cidx, old_row), t_compact = _timed(compact, a.reps)
    assert np.array_equal(old_row, keep.astype(np.uint32)) and cidx.row_bound == cidx.n_rows == len(keep)
    new_id = np.cumsum(~flags) - 1
    assert np.array_equal(cidx.list_rows, new_id[removed.list_rows].astype(np.uint32))
    sample = rng.choice(len(keep), 4096, replace=False)
    assert np.array_equal(dense.fetch_rows(sample).view(np.uint32), Xs[sample].view(np.uint32))
    lines_c = _stats_lines(compact, a.reps, "pqv_index_compact:")
    pat = re.compile(r"gather kernel ([0-9.]+) ms for ([0-9]+) row bytes .* copy of the same bytes ([0-9.]+) ms")
    got = [g for g in (pat.search(l) for l in lines_c) if g]
    t_gather, t_rcopy = [float(g.group(1)) for g in got], [float(g.group(3)) for g in got]
    row_bytes = int(got[0].group(2)) if got else 0
    reindex = lambda: pqv.IndexBuilder(pqv.Corpus.upload(Xs)).with_centroids(index).build()       # noqa: E731
    reindex()
    again, t_reindex = _timed(reindex, a.reps)
    assert again.to_bytes() == cidx.to_bytes()

    med = statistics.median
    rec = {"rows": a.rows, "dim": a.dim, "clusters": a.clusters, "fraction": a.fraction, "removed": int(flags.sum()), "reps": a.reps,
           "remove_device_ms": _mmm(t_remove),
           "route_from_parts_append_survivors_ms": _mmm(t_route), "route_upload_survivors_ms": _mmm(t_upload),
           "list_compact_kernel_ms": _mmm(t_kernel), "list_dtod_copy_ms": _mmm(t_lcopy), "list_bytes": list_bytes,
           "compact_ms": _mmm(t_compact), "upload_survivors_and_with_centroids_ms": _mmm(t_reindex),
           "rows_gather_kernel_ms": _mmm(t_gather), "rows_dtod_copy_ms": _mmm(t_rcopy), "row_bytes": row_bytes,
           "gather_tb_per_s_written": round(row_bytes / (med(t_gather) * 1e9), 3) if t_gather and med(t_gather) > 0 else None,
           "copy_tb_per_s_written": round(row_bytes / (med(t_rcopy) * 1e9), 3) if t_rcopy and med(t_rcopy) > 0 else None,
           "stats_lines": lines_r[:1] + lines_c[:1]}

    if a.search:
        Q = rng.random((a.nq, a.dim), dtype=np.float32)
        s_old, s_new = pqv.Searcher(index, corpus), pqv.Searcher(removed, corpus)
        mask = s_old.row_mask(~flags)
        masked = lambda: s_old.topk(Q, 10, a.nprobe, mask=mask)                   # noqa: E731
        plain = lambda: s_new.topk(Q, 10, a.nprobe)                               # noqa: E731
        masked(); plain()
        m, t_masked = _timed(masked, a.reps)
        p, t_plain = _timed(plain, a.reps)
        assert (m[0] == p[0]).all() and (m[1].view(np.uint32) == p[1].view(np.uint32)).all() and (m[2] == p[2]).all()
        rec.update({"nq": a.nq, "k": 10, "nprobe": a.nprobe, "topk_masked_old_searcher_ms": _mmm(t_masked),
                    "topk_removed_index_ms": _mmm(t_plain), "describe_old": s_old.describe(a.nq, 10, a.nprobe),
                    "describe_removed": s_new.describe(a.nq, 10, a.nprobe),
                    "note": "host-API topk calls (queries in, results out through the host); a masked call always runs the exact stream"})
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
