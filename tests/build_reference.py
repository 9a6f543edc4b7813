"""Checks of one index build against the reference, stage by stage (test infrastructure): the centroids against
oracle.kmeans over the build's sample, the final assignment of every row against tests/assign_exact.py under the
oracle's centroids, the lists and the blob against those assembled from that assignment.  Used by the full-size builds
of tests/test_gpu_build_full_size.py and the 1 M-row C3-shape build of tests/test_gpu_config_scale.py."""
import time

import numpy as np

import assign_exact


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def reference_blob(dim, centroids, assign, k):
    """index.rs:65-83: u32 dim, u32 n_clusters, the centroids' f32 bits, then per list its length and its rows."""
    counts = np.bincount(assign, minlength=k).astype(np.uint64)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    rows = np.argsort(assign, kind="stable").astype(np.uint32)
    body = np.empty(k + len(assign), np.uint32)
    len_at = off[:-1].astype(np.int64) + np.arange(k)
    is_row = np.ones(len(body), bool)
    is_row[len_at] = False
    body[len_at] = counts
    body[is_row] = rows
    head = np.array([dim, k], np.uint32).tobytes() + np.ascontiguousarray(centroids, np.float32).tobytes()
    return head + body.tobytes(), off, rows


def check_build_against_reference(oracle, host, gpu_blob, gpu_cent, gpu_off, gpu_rows, sample_idx, k, workers,
                                  max_iters=20, seed=42):
    """host [n, dim] f32: the rows the build saw; sample_idx: the reference's sample (oracle.index_sample), in draw
    order; gpu_*: the build's blob, centroids, list offsets and list rows.  -> (problems, record): an empty list
    when every stage equals the reference; the record has the stage times and assign_exact's exact-path counts."""
    n, dim = host.shape
    problems, rec = [], {"n": n, "dim": dim, "k": k, "workers": workers}
    t = time.time()
    sample = host[sample_idx.astype(np.int64)]    # in draw order, as sample_embeddings gathers it
    ocent, _, rec["lloyd_iters"] = oracle.kmeans(sample, k, max_iters, seed, workers)
    del sample
    rec["oracle_kmeans_s"] = round(time.time() - t, 1)
    bad_c = np.nonzero((_bits(gpu_cent) != _bits(ocent)).any(axis=1))[0]
    if len(bad_c):
        c = int(bad_c[0])
        problems.append({"centroids_differ": len(bad_c), "first": c,
                         "max_abs_diff": float(np.abs(gpu_cent[c].astype(np.float64) - ocent[c]).max())})

    assert int(gpu_off[-1]) == n and len(gpu_rows) == n and int(gpu_rows.max()) < n
    gpu_of = np.empty(n, np.uint32)
    gpu_of[gpu_rows] = np.repeat(np.arange(k, dtype=np.uint32), np.diff(gpu_off.astype(np.int64)))
    t = time.time()
    want, stats = assign_exact.nearest(host, ocent)
    rec["assign_exact_s"] = round(time.time() - t, 1)
    rec.update(exact_rows=stats["exact_rows"], max_candidates=stats["max_candidates"])
    rep = assign_exact.mismatches(host, ocent, gpu_of, want)
    if rep is not None:
        problems.append({"final_assignment": rep})
        if len(bad_c):     # is the final assignment right under the GPU's own centroids? (tells the stages apart)
            own, _ = assign_exact.nearest(host, gpu_cent)
            problems.append({"under_gpu_centroids": assign_exact.mismatches(host, gpu_cent, gpu_of, own)})

    blob, off, rows = reference_blob(dim, ocent, want, k)
    if not np.array_equal(gpu_off.astype(np.uint64), off):
        c = int(np.nonzero(gpu_off.astype(np.uint64) != off)[0][0])
        problems.append({"list_offsets_differ_first_at": c, "gpu": int(gpu_off[c]), "ref": int(off[c])})
    if not np.array_equal(gpu_rows, rows):
        p = int(np.nonzero(gpu_rows != rows)[0][0])
        problems.append({"list_rows_differ_first_at": p, "gpu": int(gpu_rows[p]), "ref": int(rows[p])})
    if gpu_blob != blob:
        p = int(np.nonzero(np.frombuffer(gpu_blob, np.uint8) != np.frombuffer(blob, np.uint8))[0][0]) \
            if len(gpu_blob) == len(blob) else -1
        problems.append({"blob_differs": True, "gpu_len": len(gpu_blob), "ref_len": len(blob), "first_byte": p})
    return problems, rec
