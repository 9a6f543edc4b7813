"""Round-3 GPU tests: the shard exchange over RCCL behind the C ABI (one rank: the collective path itself), bench.py's
self-launched multi-rank run, top-k beyond the kernels' list capacity (any k / nprobe, search.rs:56-81), tie flags of the
device-resident re-rank."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _shard_lists(rng, world, nq, k):
    """per-shard sorted top-k lists with ties across shards and some short lists (empty slots: +inf / 0xFFFFFFFF)"""
    d = np.sort(rng.integers(0, 40, size=(world, nq, k)).astype(np.float32) * 0.25, axis=2)
    r = rng.integers(0, 1 << 20, size=(world, nq, k)).astype(np.uint32)
    for w in range(world):
        for q in range(0, nq, 5):
            cut = int(rng.integers(0, k + 1))
            d[w, q, cut:] = np.inf
            r[w, q, cut:] = 0xFFFFFFFF
    return d, r


def test_shard_exchange_c_abi_one_rank_rccl(pqv):
    """pqv_shard_unique_id / comm_create / exchange with world = 1: ncclCommInitRank + ncclAllGather run for real (RCCL
    bound by the library through dlopen), the merge must equal both the torch stable-sort merge and the host merge."""
    import torch
    from pq_vector_amd import _ffi
    from pq_vector_amd.sharding import RcclShardComm, merge_gathered
    assert _ffi.lib().pqv_shard_rccl_path().decode().endswith(("librccl.so", "librccl.so.1")) or "rccl" in _ffi.lib().pqv_shard_rccl_path().decode()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    nq, k = 37, 10
    d, r = _shard_lists(rng, 1, nq, k)
    comm = RcclShardComm(0, 1, 0)
    assert _ffi.lib().pqv_shard_comm_world(comm._h) == 1 and _ffi.lib().pqv_shard_comm_rank(comm._h) == 0
    d_t = torch.from_numpy(d[0]).to(dev)
    r_t = torch.from_numpy(r[0].view(np.int32)).to(dev)
    bases = torch.tensor([1000], dtype=torch.int64, device=dev)
    out_d = torch.empty((nq, k), dtype=torch.float32, device=dev)
    out_r = torch.empty((nq, k), dtype=torch.int64, device=dev)
    for _ in range(3):          # steady state: the buffers are reused
        comm.exchange(d_t, r_t, bases, out_d, out_r)
    torch.cuda.synchronize()
    grow = np.where(r[0] == 0xFFFFFFFF, -1, r[0].astype(np.int64) + 1000)
    md, mr = merge_gathered(torch.from_numpy(d), torch.from_numpy(grow[None]), k)
    assert (_bits(out_d.cpu().numpy()) == _bits(md.numpy())).all()
    assert (out_r.cpu().numpy() == mr.numpy()).all()
    # a larger batch re-allocates the communicator's buffers
    nq2 = 300
    d2, r2 = _shard_lists(rng, 1, nq2, k)
    od2 = torch.empty((nq2, k), dtype=torch.float32, device=dev)
    or2 = torch.empty((nq2, k), dtype=torch.int64, device=dev)
    comm.exchange(torch.from_numpy(d2[0]).to(dev), torch.from_numpy(r2[0].view(np.int32)).to(dev), bases, od2, or2)
    torch.cuda.synchronize()
    hd, hr, _, _ = pqv.merge_topk(d2, r2, (r2 != 0xFFFFFFFF).sum(axis=2).astype(np.uint32))
    assert (_bits(od2.cpu().numpy()) == _bits(hd)).all()
    exp = np.where(hr == 0xFFFFFFFF, -1, hr.astype(np.int64) + 1000)
    assert (or2.cpu().numpy() == exp).all()
    comm.close()


def test_torch_rccl_exchange_one_rank_matches_merge_gathered(pqv, tmp_path):
    """The torch.distributed (backend nccl == RCCL) form bench.py cross-checks against: one rank, the collective forced,
    pqv_merge_topk_packed_device against merge_gathered."""
    import torch
    import torch.distributed as dist
    from pq_vector_amd.sharding import ShardExchange, merge_gathered
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method=f"file://{tmp_path}/rdv", rank=0, world_size=1, device_id=dev)
    try:
        rng = np.random.default_rng(6)
        nq, k = 64, 10
        d, r = _shard_lists(rng, 1, nq, k)
        x = ShardExchange(1, nq, k, dev, always_collective=True, row_bases=[7])
        od, orow = x.exchange_u32(torch.from_numpy(d[0]).to(dev), torch.from_numpy(r[0].view(np.int32)).to(dev))
        torch.cuda.synchronize()
        grow = np.where(r[0] == 0xFFFFFFFF, -1, r[0].astype(np.int64) + 7)
        md, mr = merge_gathered(torch.from_numpy(d), torch.from_numpy(grow[None]), k)
        assert (_bits(od.cpu().numpy()) == _bits(md.numpy())).all() and (orow.cpu().numpy() == mr.numpy()).all()
    finally:
        dist.destroy_process_group()



def _reject_constant(x):
    raise ValueError("non-finite number in the bench line: " + x)


def _one_compact_line(p):
    """ONE stdout line, strict JSON (no NaN / Infinity), under bench.py's 8 KB cap (round 5's 19.8 KB line was not parsed by the driver)."""
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout[-2000:]
    assert len(lines[0]) < 8192, len(lines[0])
    rec = json.loads(lines[0], parse_constant=_reject_constant)
    assert rec["full_record"] == "bench_full.json" and os.path.exists(os.path.join(ROOT, "bench_full.json"))
    return rec


@pytest.mark.timeout(600)
def test_bench_self_launches_two_ranks_on_one_gpu():
    """`python bench.py --gpus 2` exactly as the driver calls it (no launcher environment): it must start its own two
    ranks, run the sharded path end to end (gloo lets them share this box's one GPU) and print ONE JSON line."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--workload", "tiny",
                        "--steps", "3", "--warmup", "1"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=570)
    assert p.returncode == 0, p.stderr[-2000:]
    rec = _one_compact_line(p)
    assert rec["n_gpus"] == 2 and rec["steps"] == 3 and rec["config"]["shards"] == 2 and rec["value"] > 0


@pytest.mark.timeout(600)
def test_plain_bench_run_prints_the_headline_and_full_adds_the_rest(tmp_path):
    """A plain run sets up, warms up, times the steps, dumps and prints the headline; roofline, single-query latency, recall
    and the CPU baseline with its oracle parity leg come only with --full, and neither changes what the timed step returns."""
    lines, dumps = {}, {}
    for mode in ("plain", "full"):
        out = tmp_path / mode
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "tiny", "--steps", "5",
                            "--warmup", "2", "--dump-outputs", str(out)] + (["--full"] if mode == "full" else []),
                           capture_output=True, text=True, cwd=ROOT, timeout=280)
        assert p.returncode == 0, p.stderr[-2000:]
        lines[mode] = _one_compact_line(p)
        dumps[mode] = {name: np.load(out / (name + ".npy")) for name in ("distances", "rows", "n_found", "n_candidates")}
    plain, full = lines["plain"], lines["full"]
    for rec in (plain, full):
        assert rec["metric"] == "topk_queries_per_s_k10" and rec["unit"] == "queries/s" and rec["higher_is_better"] is True
        assert rec["dtype"] == "f32" and rec["steps"] == 5 and rec["warmup"] == 2 and rec["value"] > 0
        assert rec["value"] == pytest.approx(64 * 1e3 / rec["ms_per_step"], rel=1e-4)
    for key in ("roofline", "cpu_baseline", "single_query", "recall_at_k", "ms_per_step_serial"):
        assert key not in plain, key
        assert key in full, key
    assert full["cpu_baseline"]["parity_ok"] is True and full["roofline"]["bound"] == "hbm"
    for name, a in dumps["plain"].items():
        assert np.array_equal(a.view(np.uint8), dumps["full"][name].view(np.uint8)), name


def test_cpp_host_mirror_example_matches_the_oracle(oracle, tmp_path):
    """pq-vector_amd/host/pqv.hpp (the header-only C++ mirror of IndexBuilder / TopkBuilder over the C ABI) through its example
    program: the index it builds and the answers it prints must be the oracle's on the same data."""
    exe = os.path.join(ROOT, "pq-vector_amd", "host", "example_topk")
    assert os.path.exists(exe), "built by make -C pq-vector_amd/csrc (__graft_entry__.build)"
    out = str(tmp_path / "example.bin")
    p = subprocess.run([exe, out], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    raw = open(out, "rb").read()
    n, dim, blob_len, n_hits = np.frombuffer(raw, dtype=np.uint64, count=4)
    n, dim, blob_len, n_hits = int(n), int(dim), int(blob_len), int(n_hits)
    off = 32
    data = np.frombuffer(raw, dtype=np.float32, count=n * dim, offset=off).reshape(n, dim); off += n * dim * 4
    query = np.frombuffer(raw, dtype=np.float32, count=dim, offset=off); off += dim * 4
    blob = raw[off:off + blob_len]; off += blob_len
    hits = np.frombuffer(raw, dtype=np.uint32, count=2 * n_hits, offset=off).reshape(n_hits, 2)
    oidx = oracle.build_index(np.ascontiguousarray(data), n_clusters=16, workers=os.cpu_count() or 1)     # the example builds with workers = 0: this host's CPUs
    assert oidx.to_bytes() == blob
    orows, odist, onf, _ = oidx.topk_batch(np.ascontiguousarray(data), query.reshape(1, -1).copy(), 5, 4)
    assert int(onf[0]) == n_hits == 5
    assert (hits[:, 0] == orows[0]).all() and (hits[:, 1] == odist[0].view(np.uint32)).all()


def test_bench_c4_two_ranks_with_a_small_shard():
    """BASELINE configs[3]'s code path -- one shard and one index per rank, the whole batch searched on every shard, one exchange
    per step -- with two ranks of 1 M rows each on this box's one GPU (gloo): the line must carry both ranks' step times and the
    exchange's share.  (No multi-GPU hardware has run this yet: the 1 -> 8 curve is the driver's to measure.)"""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--workload", "c4",
                        "--rows-per-rank", "1000000", "--steps", "5", "--warmup", "1", "--no-cpu", "--full"],
                       capture_output=True, text=True, env=env, cwd=ROOT, timeout=570)
    assert p.returncode == 0, p.stderr[-2000:]
    rec = _one_compact_line(p)
    assert rec["n_gpus"] == 2 and rec["config"]["shards"] == 2 and rec["config"]["rows_per_gpu"] == 1000000 and rec["value"] > 0
    assert rec["scaling"] == "weak" and len(rec["per_rank_ms_per_step"]["ranks"]) == 2
    assert rec["per_rank_ms_per_step"]["max"] <= rec["ms_per_step"] * 1.5 + 1.0
    assert rec["exchange"]["ranks"] == 2 and 0.0 < rec["exchange"]["share_of_step"]


def test_bench_two_ranks_share_one_parquet_file_by_row_group_ranges():
    """BASELINE configs[3]'s partition unit: ONE Parquet file, one row-group range per rank (sharding.shard_row_groups +
    parquet_io.load_embedding_column(row_groups=...)), a shard index per rank, the lists exchanged -- two ranks on this box's one
    GPU (gloo).  The line's parity leg: with every list probed the merged answer carries the same file-global row ids and
    distance bits as a single-shard search of the whole file."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--from-parquet",
                        "--rows-per-rank", "150000", "--nq", "64", "--steps", "3", "--warmup", "1", "--parity-queries", "32"],
                       capture_output=True, text=True, env=env, cwd=ROOT, timeout=570)
    assert p.returncode == 0, p.stderr[-3000:]
    rec = _one_compact_line(p)
    cfg = rec["config"]
    assert rec["n_gpus"] == 2 and cfg["shards"] == 2 and cfg["row_groups"] == 9 and rec["value"] > 0
    (a0, a1), (b0, b1) = cfg["row_group_ranges"]
    assert a0 == 0 and a1 == b0 and b1 == 9 and cfg["row_bases"][0] == 0 and cfg["row_bases"][1] == cfg["shard_rows"][0]
    assert sum(cfg["shard_rows"]) == 300000 and cfg["shard_rows"][0] != cfg["shard_rows"][1]      # cut at a row-group boundary, not at n / 2
    assert rec["parity"]["ok"] and rec["parity"]["queries_checked"] == 32
    assert rec["parity"]["global_row_ids_identical"] and rec["parity"]["dist_bit_identical"]
    assert "data pages" in rec["per_rank"]["loader_path"]


# Ranks of the many-rank bench runs below.  They all share this box's one GPU, and together with the test process at most
# five processes hold it at once.  (The eight-rank line's size is checked on the CPU: test_bench_line.py.)
SHARED_GPU_RANKS = 4


@pytest.mark.timeout(900)
def test_bench_many_ranks_share_one_parquet_file():
    """The --gpus N job shape for N > 2 on this box's one GPU (gloo): N row-group cuts from one footer, N shard indexes, the N-way
    merge.  With every list probed the merged answer equals a single-shard search of the whole file; the line obeys the
    compact-line rule with every rank's figures on it."""
    w = SHARED_GPU_RANKS
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(w), "--backend", "gloo", "--from-parquet",
                        "--rows-per-rank", "100000", "--nq", "64", "--steps", "3", "--warmup", "1", "--parity-queries", "32"],
                       capture_output=True, text=True, env=env, cwd=ROOT, timeout=870)
    assert p.returncode == 0, p.stderr[-3000:]
    rec = _one_compact_line(p)
    cfg = rec["config"]
    assert rec["n_gpus"] == w and cfg["shards"] == w and cfg["row_groups"] == 4 * w + 1 and rec["value"] > 0
    rng = cfg["row_group_ranges"]
    assert len(rng) == w and rng[0][0] == 0 and rng[-1][1] == 4 * w + 1 and all(rng[i][1] == rng[i + 1][0] for i in range(w - 1))
    assert all(hi > lo for lo, hi in rng) and sum(cfg["shard_rows"]) == w * 100000
    assert cfg["row_bases"] == [sum(cfg["shard_rows"][:i]) for i in range(w)]
    assert len(set(cfg["shard_rows"])) > 1                    # cuts at row-group boundaries, not at n / w
    assert rec["parity"]["ok"] and rec["parity"]["queries_checked"] == 32
    assert rec["parity"]["global_row_ids_identical"] and rec["parity"]["dist_bit_identical"]
    assert len(rec["per_rank"]["load_s"]) == w and rec["exchange"]["ranks"] == w


@pytest.mark.timeout(900)
def test_bench_c4_many_ranks_with_small_shards():
    """BASELINE configs[3] as the driver launches it (--gpus N, N > 2), 250 k-row shards on this box's one GPU (gloo): one shard
    and one index per rank, the whole batch on every shard, one exchange per step; only rank 0 may run the CPU baseline, and it
    does not at N > 1 (the brief: rank 0 at N = 1 only)."""
    w = SHARED_GPU_RANKS
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(w), "--backend", "gloo", "--workload", "c4",
                        "--rows-per-rank", "250000", "--steps", "5", "--warmup", "1", "--full"],
                       capture_output=True, text=True, env=env, cwd=ROOT, timeout=870)
    assert p.returncode == 0, p.stderr[-3000:]
    rec = _one_compact_line(p)
    assert rec["n_gpus"] == w and rec["config"]["shards"] == w and rec["config"]["rows_per_gpu"] == 250000 and rec["value"] > 0
    assert rec["scaling"] == "weak" and len(rec["per_rank_ms_per_step"]["ranks"]) == w
    assert rec["exchange"]["ranks"] == w and 0.0 < rec["exchange"]["share_of_step"]
    assert "cpu_baseline" not in rec and p.stderr.count("oracle -O3") == 0


@pytest.mark.parametrize("k,nprobe", [(1024, 4), (1500, 6), (3000, 3), (10, 1500)])
def test_topk_beyond_the_kernel_list_capacity(pqv, oracle, k, nprobe):
    """search.rs:56-81 accepts any NonZeroUsize for k and nprobe.  k >= 1024 (no runner-up slot in the kernels' lists) and
    min(nprobe, n_clusters) > 1024 take pqv_topk's host-replayed path: distances on the GPU, selection by the reference's
    heap -- ids and distance bits equal to the oracle, tie-heavy data included."""
    rng = np.random.default_rng(k + nprobe)
    if nprobe > 1024:
        n, dim, kc = 6000, 8, 2000
        data = rng.random((n, dim), dtype=np.float32)
    else:
        n, dim, kc = 9000, 16, 6
        data = rng.integers(0, 4, size=(n, dim)).astype(np.float32)       # massive ties
    queries = data[:3] + (0.0 if nprobe <= 1024 else 0.01)
    queries = np.ascontiguousarray(queries, dtype=np.float32)
    corpus = pqv.Corpus.upload(data)
    index = pqv.IndexBuilder(corpus).n_clusters(kc).workers(4).max_iters(3).build()
    oidx = oracle.index_from_bytes(index.to_bytes())
    s = pqv.Searcher(index, corpus)
    rows, dist, nf, nc = s.topk(queries, k, nprobe)
    orows, odist, onf, onc = oidx.topk_batch(data, queries, k, nprobe)
    assert (nf == onf).all() and (nc == onc).all()
    for q in range(len(queries)):
        m = int(nf[q])
        assert (_bits(dist[q, :m]) == _bits(odist[q, :m])).all()
        assert (rows[q, :m] == orows[q, :m]).all()
    assert (s.probe(queries[0], nprobe) == np.asarray(oidx.find_closest_centroids(queries[0], nprobe))).all()
    # the asynchronous device entry points report the limit instead of going to the host
    import torch
    dev = torch.device("cuda", 0)
    q_t = torch.from_numpy(queries).to(dev)
    r_t = torch.empty((len(queries), k), dtype=torch.int32, device=dev)
    d_t = torch.empty((len(queries), k), dtype=torch.float32, device=dev)
    if k > 1024 or min(nprobe, kc) > 1024:
        with pytest.raises(pqv.PqvError):
            s.topk_device(q_t.data_ptr(), len(queries), k, nprobe, r_t.data_ptr(), d_t.data_ptr())


def test_rerank_device_flags_mark_the_folds_that_need_the_heap(pqv, oracle):
    """pqv_rerank_device_flags: the device-resident fold keeps (d2, arrival) order; its sticky flag must be set exactly
    when two of the k results, or the k-th and the first excluded row, tie in some fold -- the only case in which the
    reference's heap (exec.rs:474-481) may answer differently.  Unflagged runs must equal the oracle id for id."""
    import torch
    from pq_vector_amd import _ffi
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(21)
    n, dim, k = 8192, 64, 10
    for case in ("distinct", "dup_inside", "dup_at_boundary"):
        emb = rng.random((n, dim), dtype=np.float32)
        q = rng.random(dim, dtype=np.float32)
        d2 = ((emb.astype(np.float64) - q) ** 2).sum(axis=1)
        order = np.argsort(d2, kind="stable")
        if case == "dup_inside":
            emb[order[3]] = emb[order[2]]                  # two of the k results tie
        elif case == "dup_at_boundary":
            emb[order[k]] = emb[order[k - 1]]              # the k-th and the runner-up tie
        arrival = rng.permutation(n).astype(np.uint32)
        emb_t = torch.from_numpy(emb[arrival]).to(dev)
        ids_t = torch.from_numpy(arrival.astype(np.int32)).to(dev)
        q_t = torch.from_numpy(q).to(dev)
        io_r = torch.zeros((k,), dtype=torch.int32, device=dev)
        io_d = torch.zeros((k,), dtype=torch.float32, device=dev)
        io_c = torch.zeros((1,), dtype=torch.int32, device=dev)
        flag = torch.zeros((1,), dtype=torch.int32, device=dev)
        for b in range(0, n, 2048):
            rc = _ffi.lib().pqv_rerank_device_flags(0, _ffi.vp(q_t.data_ptr()), _ffi.vp(emb_t[b:b + 2048].data_ptr()),
                                                    _ffi.vp(ids_t[b:b + 2048].data_ptr()), 2048, dim, k, pqv.PQV_L2SQ_SEQ,
                                                    _ffi.vp(io_r.data_ptr()), _ffi.vp(io_d.data_ptr()), _ffi.vp(io_c.data_ptr()),
                                                    _ffi.vp(flag.data_ptr()), None)
            assert rc == 0, _ffi.lib().pqv_last_error()
        torch.cuda.synchronize()
        orow, od2 = oracle.topk_df(emb, arrival, q, k)
        got_r, got_d = io_r.cpu().numpy().view(np.uint32), io_d.cpu().numpy()
        assert (_bits(got_d) == _bits(od2)).all()
        if case == "distinct":
            assert int(flag.item()) == 0 and (got_r == orow).all()
        else:
            assert int(flag.item()) == 1
            # the flagged run goes through pqv_rerank, which replays the heap: equal to the reference
            state = None
            for b in range(0, n, 2048):
                state = pqv.rerank_batch(q, emb[arrival[b:b + 2048]], k, state=state, ids=arrival[b:b + 2048])
            hr, hd = pqv.rerank_finish(state)
            assert (hr == orow).all() and (_bits(hd) == _bits(od2)).all()
