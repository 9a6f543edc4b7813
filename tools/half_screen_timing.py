#!/usr/bin/env python3
"""Times the screened route over f16 rows (rerank_mode 2: screen_h_kernel + survivor_h_kernel) on one GPU against
  parent   the PARENT commit's library (--parent-lib, through PQV_LIB_PATH) on the same f16 corpus: stream_h_kernel
  f32      as a yardstick only, this tree's f32 searcher by rule (the int8-screened route) on the widened rows
at 1 M x 768, 1024 lists, nprobe 32, k 10, 256 queries per step through pqv_topk_device -- tools/half_timing.py's method: a
process per side on the same seeded data and index, the sides alternating `--rounds` times, `--blocks` blocks of `--steps` steps
between device synchronisations after a warm-up, row ids and distance bits compared through a digest.  Prints one JSON line and
writes it to --out (default profiles/half_screen_timing.json)."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDES = ("parent", "screen", "f32")


def worker(a):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import pq_vector_amd as pqv

    rng = np.random.default_rng(11)
    half = rng.standard_normal((a.rows, a.dim), dtype=np.float32).astype(np.float16)
    queries = rng.standard_normal((a.nq, a.dim), dtype=np.float32)
    f32_corpus = pqv.Corpus.upload(half.astype(np.float32))
    index = pqv.IndexBuilder(f32_corpus).n_clusters(a.clusters).build()
    if a.side == "f32":
        s = pqv.Searcher(index, f32_corpus)
    else:
        del f32_corpus
        s = pqv.Searcher(index, pqv.Corpus.upload(half))
        if a.side == "screen":
            s.set_option("rerank_mode", 2)
    q = torch.from_numpy(queries).cuda()
    rows = torch.zeros((a.nq, a.k), dtype=torch.int32, device="cuda")
    dist = torch.zeros((a.nq, a.k), dtype=torch.float32, device="cuda")

    def step():
        s.topk_device(q.data_ptr(), a.nq, a.k, a.nprobe, rows.data_ptr(), dist.data_ptr())

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    c0 = s.counters()
    blocks = []
    for _ in range(a.blocks):
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
        torch.cuda.synchronize()
        blocks.append((time.perf_counter() - t0) * 1e3 / a.steps)
    c1 = s.counters()
    digest = hashlib.sha256(rows.cpu().numpy().tobytes() + dist.cpu().numpy().tobytes()).hexdigest()
    print(json.dumps({"side": a.side, "step_ms_blocks": blocks, "digest": digest, "dispatch": s.describe(a.nq, a.k, a.nprobe),
                      "screened_pairs": c1["screened_pairs"] - c0["screened_pairs"], "screen_survivors": c1["screen_survivors"] - c0["screen_survivors"]}))


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "half_screen_timing.json"))
    ap.add_argument("--side", choices=SIDES, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.side:
        return worker(a)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("--parent-lib must name the parent commit's libpqv_hip.so")
    shape = [f"--{n}={getattr(a, n)}" for n in ("rows", "dim", "clusters", "nprobe", "k", "nq", "steps", "warmup", "blocks")]
    runs = {side: [] for side in SIDES}
    last = {}
    for _ in range(a.rounds):
        for side in SIDES:
            env = dict(os.environ)
            env.pop("PQV_LIB_PATH", None)
            if side == "parent":
                env["PQV_LIB_PATH"] = os.path.abspath(a.parent_lib)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--side", side] + shape, env=env, check=True,
                                 stdout=subprocess.PIPE, text=True).stdout
            last[side] = json.loads(out.strip().splitlines()[-1])
            runs[side].append(last[side]["step_ms_blocks"])
    if len({last[side]["digest"] for side in SIDES}) != 1:
        sys.exit("the sides returned different rows or distance bits")

    def summary(side):
        meds = [statistics.median(r) for r in runs[side]]
        every = [t for r in runs[side] for t in r]
        return {"round_medians_ms": [round(m, 4) for m in meds], "step_ms": round(statistics.median(every), 4),
                "spread_of_round_medians_ms": round(max(meds) - min(meds), 4), "dispatch": last[side]["dispatch"]}

    parent, screen, f32 = summary("parent"), summary("screen"), summary("f32")
    rec = {"shape": {n: getattr(a, n) for n in ("rows", "dim", "clusters", "nprobe", "k", "nq")},
           "timing": {"steps_per_block": a.steps, "blocks": a.blocks, "rounds": a.rounds, "warmup_steps": a.warmup,
                      "clock": "host clock around `steps` pqv_topk_device calls and a device synchronise; sides alternate, one process each"},
           "f16_parent_stream": parent, "f16_screened_rerank_mode_2": screen, "f32_yardstick_by_rule": f32,
           "survivors_over_screened_pairs": round(last["screen"]["screen_survivors"] / max(1, last["screen"]["screened_pairs"]), 5),
           "parent_over_screened": round(parent["step_ms"] / screen["step_ms"], 3),
           "screened_over_f32_yardstick": round(screen["step_ms"] / f32["step_ms"], 3),
           "results_identical": True,
           "faster_than_parent_beyond_its_spread": screen["step_ms"] < parent["step_ms"] - parent["spread_of_round_medians_ms"]}
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
