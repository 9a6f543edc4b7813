#!/usr/bin/env python3
"""Times index append against a full build on one GPU, in one process: at a given shape (default C2's: 1 M x 128,
100 clusters)
  1. pqv_index_build over all rows,
  2. pqv_index_append of the last `--tail` rows onto an index built over the rows before them,
  3. the splice kernel alone between HIP events, beside a device-to-device copy of the same list bytes on the same stream
     (the library's PQV_APPEND_STATS=1 line, switched on for these calls only).
Prints one JSON line; --out also writes it to a file.  The appended index is compared with a from-scratch nearest-centroid
assignment on a row sample through Index.assign, so a wrong result cannot be timed."""
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


def _stats_lines(fn, reps):
    """Runs fn() `reps` times with PQV_APPEND_STATS=1 and the process' stderr in a file; -> the library's lines."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        os.environ["PQV_APPEND_STATS"] = "1"
        try:
            for _ in range(reps):
                fn()
        finally:
            del os.environ["PQV_APPEND_STATS"]
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        return [l for l in f.read().decode().splitlines() if l.startswith("pqv_index_append:")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--clusters", type=int, default=100)
    ap.add_argument("--tail", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    import pq_vector_amd as pqv

    rng = np.random.default_rng(2)
    X = rng.random((a.rows, a.dim), dtype=np.float32)
    n0 = a.rows - a.tail
    corpus = pqv.Corpus.create(a.rows, a.dim)
    corpus.append(X[:n0])
    build = lambda: pqv.IndexBuilder(corpus).n_clusters(a.clusters).build()     # noqa: E731
    build()                                                                     # warm-up: code objects, scratch, pools
    old, _ = _timed(build, 1)
    corpus.append(X[n0:])
    _, t_build = _timed(build, a.reps)
    old.append(corpus)                                                          # warm-up of the append's own kernels
    new, t_append = _timed(lambda: old.append(corpus), a.reps)

    lines = _stats_lines(lambda: old.append(corpus), a.reps)
    pat = re.compile(r"splice kernel ([0-9.]+) ms for ([0-9]+) list bytes .* copy of the same bytes ([0-9.]+) ms")
    got = [pat.search(l) for l in lines]
    splice = [float(g.group(1)) for g in got if g]
    copy = [float(g.group(3)) for g in got if g]
    nbytes = int(got[0].group(2)) if got and got[0] else 0

    # the appended index is what its definition says, on a sample of the new rows and on the old lists
    assert new.n_rows == a.rows and new.row_bound == a.rows
    off_old, off_new = old.list_offsets.astype(np.int64), new.list_offsets.astype(np.int64)
    rows_old, rows_new = old.list_rows, new.list_rows
    cluster_of = np.empty(a.rows, np.uint32)
    cluster_of[rows_new] = np.repeat(np.arange(a.clusters, dtype=np.uint32), np.diff(off_new))
    for c in range(a.clusters):
        seg = rows_new[off_new[c]:off_new[c + 1]]
        assert np.array_equal(seg[:off_old[c + 1] - off_old[c]], rows_old[off_old[c]:off_old[c + 1]])
        assert (np.diff(seg.astype(np.int64)) > 0).all()
    assert np.array_equal(cluster_of[n0:], old.assign(corpus, n0, a.tail))

    med = statistics.median
    rec = {"rows": a.rows, "dim": a.dim, "clusters": a.clusters, "tail": a.tail, "reps": a.reps,
           "build_all_ms": {"median": round(med(t_build), 3), "min": round(min(t_build), 3), "max": round(max(t_build), 3)},
           "append_tail_ms": {"median": round(med(t_append), 3), "min": round(min(t_append), 3), "max": round(max(t_append), 3)},
           "splice_kernel_ms": {"median": med(splice), "min": min(splice), "max": max(splice)} if splice else None,
           "dtod_copy_ms": {"median": med(copy), "min": min(copy), "max": max(copy)} if copy else None,
           "list_bytes": nbytes,
           "splice_gb_per_s_written": round(nbytes / (med(splice) * 1e6), 1) if splice and med(splice) > 0 else None,
           "stats_lines": lines[:2]}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
