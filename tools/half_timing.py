#!/usr/bin/env python3
"""Times the exact stream over f16 rows against the f32 exact stream on the widened rows, on one GPU:
  f16   this tree's library, a searcher over an f16 corpus (stream_h_kernel), pqv_topk_device
  f32   the PARENT commit's library (--parent-lib: a build of the commit before half-precision corpora), a searcher over the
        widened rows under rerank_mode = 1 (stream_kernel), pqv_topk_device
at 1 M x 768, 1024 lists, nprobe 32, k 10, 256 queries per step.  Each side runs in a process of its own (one library per
process) on the same seeded data and the same index (built on the device from the widened rows); the sides ALTERNATE, `--rounds`
times each, and every process times `--blocks` blocks of `--steps` steps between device synchronisations after a warm-up.  The
two sides' row ids and distance bits are compared through a digest, so a wrong result cannot be timed.  Prints one JSON line and
writes it to --out (default profiles/half_timing.json): per side the block medians of every round, their overall median and
spread, and ratio = f32 step / f16 step."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def worker(a):
    import ctypes
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from pq_vector_amd import _ffi
    if a.side == "f32":      # the parent's library has none of the f16 entry points: bind what it exports
        have = ctypes.CDLL(_ffi.LIB_PATH)
        for name in [n for n in _ffi.SIGNATURES if not hasattr(have, n)]:
            del _ffi.SIGNATURES[name]
    import pq_vector_amd as pqv

    rng = np.random.default_rng(11)
    half = rng.standard_normal((a.rows, a.dim), dtype=np.float32).astype(np.float16)
    wide = half.astype(np.float32)
    queries = rng.standard_normal((a.nq, a.dim), dtype=np.float32)
    f32_corpus = pqv.Corpus.upload(wide)
    index = pqv.IndexBuilder(f32_corpus).n_clusters(a.clusters).build()
    if a.side == "f16":
        del f32_corpus
        corpus = pqv.Corpus.upload(half)
        s = pqv.Searcher(index, corpus)
    else:
        corpus = f32_corpus
        s = pqv.Searcher(index, corpus).set_option("rerank_mode", 1)
    q = torch.from_numpy(queries).cuda()
    rows = torch.zeros((a.nq, a.k), dtype=torch.int32, device="cuda")
    dist = torch.zeros((a.nq, a.k), dtype=torch.float32, device="cuda")

    def step():
        s.topk_device(q.data_ptr(), a.nq, a.k, a.nprobe, rows.data_ptr(), dist.data_ptr())

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    blocks = []
    for _ in range(a.blocks):
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
        torch.cuda.synchronize()
        blocks.append((time.perf_counter() - t0) * 1e3 / a.steps)
    digest = hashlib.sha256(rows.cpu().numpy().tobytes() + dist.cpu().numpy().tobytes()).hexdigest()
    print(json.dumps({"side": a.side, "step_ms_blocks": blocks, "digest": digest, "dispatch": s.describe(a.nq, a.k, a.nprobe)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libpqv_hip.so built from the parent commit")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--clusters", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nq", type=int, default=256)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "half_timing.json"))
    ap.add_argument("--side", choices=["f16", "f32"], help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.side:
        return worker(a)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("--parent-lib must name the parent commit's libpqv_hip.so")
    shape = [f"--{n}={getattr(a, n)}" for n in ("rows", "dim", "clusters", "nprobe", "k", "nq", "steps", "warmup", "blocks")]
    runs = {"f16": [], "f32": []}
    digests = set()
    info = {}
    for _ in range(a.rounds):
        for side in ("f16", "f32"):
            env = dict(os.environ)
            if side == "f32":
                env["PQV_LIB_PATH"] = os.path.abspath(a.parent_lib)
            else:
                env.pop("PQV_LIB_PATH", None)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--side", side] + shape, env=env, check=True,
                                 stdout=subprocess.PIPE, text=True).stdout
            rec = json.loads(out.strip().splitlines()[-1])
            runs[side].append(rec["step_ms_blocks"])
            digests.add(rec["digest"])
            info[side] = rec["dispatch"]
    if len(digests) != 1:
        sys.exit("the f16 and f32 searchers returned different rows or distance bits")

    def summary(rounds):
        meds = [statistics.median(r) for r in rounds]
        every = [t for r in rounds for t in r]
        return {"round_medians_ms": [round(m, 4) for m in meds], "step_ms": round(statistics.median(every), 4),
                "min_ms": round(min(every), 4), "max_ms": round(max(every), 4),
                "spread_of_round_medians": round((max(meds) - min(meds)) / statistics.median(meds), 4)}

    f16, f32 = summary(runs["f16"]), summary(runs["f32"])
    row_bytes = a.nq * a.nprobe * (a.rows / a.clusters) * a.dim       # values a step reads, by shape (mean list length)
    rec = {"shape": {n: getattr(a, n) for n in ("rows", "dim", "clusters", "nprobe", "k", "nq")},
           "timing": {"steps_per_block": a.steps, "blocks": a.blocks, "rounds": a.rounds, "warmup_steps": a.warmup,
                      "clock": "host clock around `steps` pqv_topk_device calls and a device synchronise; sides alternate, one process each"},
           "f16_this_tree": dict(f16, dispatch=info["f16"], row_gb_per_s=round(row_bytes * 2 / (f16["step_ms"] * 1e6), 1)),
           "f32_parent_rerank_mode_1": dict(f32, dispatch=info["f32"], row_gb_per_s=round(row_bytes * 4 / (f32["step_ms"] * 1e6), 1)),
           "ratio_f32_over_f16": round(f32["step_ms"] / f16["step_ms"], 4),
           "results_identical": True,
           "f16_not_slower_beyond_spread": f16["step_ms"] <= f32["step_ms"] * (1 + max(f16["spread_of_round_medians"], f32["spread_of_round_medians"]))}
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
