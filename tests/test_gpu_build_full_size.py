"""The index BUILD at BASELINE.json's full C3 / C4 sizes against the reference, every row.

bench.py's build -- IndexBuilder(corpus).n_clusters(1024).max_iters(20).seed(42).workers(os.cpu_count()) on 10 M (C3)
or 12.5 M (the C4 shard) x 768 rows generated on the device -- is compared stage by stage with the reference, never
with the GPU's own intermediate results:
  * centroids: the 100 000-row sample (index.rs:222-242, index::sample's rejection branch at these sizes), then
    oracle.kmeans over it with the same `workers` (the reference's chunk count): k-means++ over a 50 000-row subset,
    1024 rounds, 20 Lloyd iterations.  Bit for bit.
  * final assignment: all n rows against tests/assign_exact.py under the ORACLE's centroids (the f32 chain's answer,
    decided by an f64 GEMM with a rigorous rounding bound and the exact chain where the bound cannot decide).
  * lists and blob: list_offsets == prefix sums of the per-cluster counts, list_rows == the stable sort by cluster,
    to_bytes() == the blob assembled from the oracle's centroids and those lists (index.rs:65-83).
(tests/build_reference.py.)  The full oracle build would spend minutes per case in the final assignment alone; the f64 check takes seconds."""
import gc
import os
import time

import numpy as np
import pytest

from build_reference import check_build_against_reference

pytestmark = pytest.mark.gpu


def _full_size_build(pqv, oracle, name, data_kind):
    import torch
    import bench
    n, dim, kc, _, _ = bench.WORKLOADS[name]
    workers = os.cpu_count() or 1
    dev = torch.device("cuda", 0)
    t0 = time.time()
    if data_kind == "mixture":
        corpus_t = bench.synth_mixture(torch, dev, 1234, n, dim, kc)
    else:
        corpus_t = bench.synth(torch, dev, 1234, n, dim)
    torch.cuda.synchronize()
    corpus = pqv.Corpus.from_device_ptr(corpus_t.data_ptr(), n, dim, device=0, keepalive=corpus_t)
    index = pqv.IndexBuilder(corpus).n_clusters(kc).max_iters(20).seed(42).workers(workers).build()
    blob, cent, off, rows = index.to_bytes(), index.centroids, index.list_offsets, index.list_rows
    index.close()
    corpus.close()
    host = corpus_t.cpu().numpy()                  # downloaded once
    del corpus_t, corpus, index
    gc.collect()
    torch.cuda.empty_cache()
    sample_idx, branch = oracle.index_sample(oracle.rng(42), n, 100_000)
    assert branch == 2                             # rejection: the branch C3 / C4 / C5 builds take
    problems, rec = check_build_against_reference(oracle, host, blob, cent, off, rows, sample_idx, kc, workers)
    del host
    gc.collect()
    rec["wall_s"] = round(time.time() - t0, 1)
    print(f"\n{name} {data_kind}: {rec}")
    assert not problems, problems
    return rec


@pytest.mark.timeout(1800)
def test_c3_full_size_build_uniform_equals_reference(pqv, oracle):
    _full_size_build(pqv, oracle, "c3", "uniform")


@pytest.mark.timeout(1800)
def test_c3_full_size_build_mixture_equals_reference(pqv, oracle):
    _full_size_build(pqv, oracle, "c3", "mixture")


@pytest.mark.timeout(1800)
def test_c4_shard_full_size_build_equals_reference(pqv, oracle):
    _full_size_build(pqv, oracle, "c4", "uniform")
