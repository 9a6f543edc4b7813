#!/usr/bin/env python3
"""Times the index build straight from f16 rows against the only thing the parent commit can do for such a column,
on one GPU:
  f16   this tree's library: pqv_index_build_f16 over the f16 column (assign_h_wide_kernel: the rows as stored are the operand)
  f32   the PARENT commit's library (--parent-lib): pqv_index_build over the column widened to f32 -- twice the HBM --, whose
        final assignment first writes a centred f16 image of every row and then contracts
at 2 M x 768, 1024 clusters, default iterations.  Each side runs in a process of its own (one library per process) on the same
seeded data, generated on the device; the sides ALTERNATE, `--rounds` times each, and every process times `--builds` builds after
one warm-up build.  Per build: the whole call (host clock), the final-assignment phase and the contraction kernel's own time
(pqv_index_build_stats: BS_FINAL_ASSIGN_S, BS_WIDE_KERNEL_S, HIP events around the kernel).  The index blobs are compared through a
digest, so a wrong build cannot be timed.  One more process per side runs under PQV_VERBOSE=1 (not timed) for the line that
reports the share of rows resolved exactly.  Prints one JSON line and writes it to --out (default
profiles/half_build_timing.json).  The condition it records: the f16 final assignment is not slower than the parent's f32 one
beyond the parent's own run-to-run range (max - min over its builds).
--parent-side f16 times the parent's pqv_index_build_f16 over the same f16 column instead (a parent that has the call): the same
build on both libraries, for a change that must leave it as fast as it was; the record then says so in its keys."""
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
    import torch
    sys.path.insert(0, ROOT)
    from pq_vector_amd import _ffi
    if os.environ.get("PQV_LIB_PATH"):      # a parent's library may lack the _f16 build entry points: bind what it exports
        have = ctypes.CDLL(_ffi.LIB_PATH)
        for name in [n for n in _ffi.SIGNATURES if not hasattr(have, n)]:
            del _ffi.SIGNATURES[name]
    import pq_vector_amd as pqv

    torch.manual_seed(11)
    rows = torch.randn((a.rows, a.dim), device="cuda", dtype=torch.float32).to(torch.float16)
    if a.side == "f32":
        rows = rows.to(torch.float32)
    torch.cuda.synchronize()
    corpus = pqv.Corpus.from_device(rows)
    builder = pqv.IndexBuilder(corpus).n_clusters(a.clusters).workers(a.workers)
    build = builder.build_f16 if a.side == "f16" else builder.build
    recs, digest = [], None
    for i in range(a.builds + 1):
        t0 = time.perf_counter()
        index = build()
        whole = time.perf_counter() - t0
        st = (ctypes.c_double * 10)()
        _ffi.lib().pqv_index_build_stats(st, 10)
        if i:                # (build 0 warms the code objects and the allocator up)
            recs.append({"build_s": whole, "final_assign_s": st[3], "wide_kernel_s": st[8], "final_form": int(st[5]), "wide_launches": int(st[9])})
        digest = hashlib.sha256(index.to_bytes()).hexdigest()
    print(json.dumps({"side": a.side, "builds": recs, "digest": digest}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libpqv_hip.so built from the parent commit")
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--clusters", type=int, default=1024)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--builds", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "half_build_timing.json"))
    ap.add_argument("--parent-side", choices=["f32", "f16"], default="f32",
                    help="what the parent's library builds: the widened f32 column (default) or the f16 column itself")
    ap.add_argument("--side", choices=["f16", "f32"], help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.side:
        return worker(a)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("--parent-lib must name the parent commit's libpqv_hip.so")
    shape = [f"--{n}={getattr(a, n)}" for n in ("rows", "dim", "clusters", "workers", "builds")]

    def run(who, verbose):
        env = dict(os.environ)
        side = "f16" if who == "f16" else a.parent_side
        if who == "f32":
            env["PQV_LIB_PATH"] = os.path.abspath(a.parent_lib)
        else:
            env.pop("PQV_LIB_PATH", None)
        if verbose:
            env["PQV_VERBOSE"] = "1"
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--side", side] + shape, env=env, check=True,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE if verbose else None, text=True)
        return json.loads(p.stdout.strip().splitlines()[-1]), (p.stderr if verbose else "")

    runs = {"f16": [], "f32": []}
    digests = set()
    for _ in range(a.rounds):
        for side in ("f16", "f32"):
            rec, _err = run(side, False)
            runs[side].append(rec["builds"])
            digests.add(rec["digest"])
    if len(digests) != 1:
        sys.exit("the f16 build and the parent's build gave different index blobs")
    lines = {}
    for side in ("f16", "f32"):
        rec, err = run(side, True)
        digests.add(rec["digest"])
        hits = [l for l in err.splitlines() if "evaluated exactly" in l and str(a.rows) in l]
        lines[side] = hits[-1] if hits else None
    if len(digests) != 1:
        sys.exit("a PQV_VERBOSE build gave a different index blob")

    def summary(rounds, key):
        every = [b[key] * 1e3 for r in rounds for b in r]
        return {"median_ms": round(statistics.median(every), 3), "min_ms": round(min(every), 3), "max_ms": round(max(every), 3),
                "round_medians_ms": [round(statistics.median([b[key] * 1e3 for b in r]), 3) for r in rounds]}

    def side_rec(rounds):
        return {"final_assign": summary(rounds, "final_assign_s"), "wide_kernel": summary(rounds, "wide_kernel_s"),
                "build": summary(rounds, "build_s"), "final_form": sorted({b["final_form"] for r in rounds for b in r}),
                "wide_launches": sorted({b["wide_launches"] for r in rounds for b in r})}

    f16, f32 = side_rec(runs["f16"]), side_rec(runs["f32"])
    parent_range = f32["final_assign"]["max_ms"] - f32["final_assign"]["min_ms"]
    rec = {"shape": {n: getattr(a, n) for n in ("rows", "dim", "clusters", "workers")},
           "timing": {"builds_per_process": a.builds, "rounds": a.rounds, "warmup_builds": 1,
                      "clock": "pqv_index_build_stats of each build (host clock of the phase; HIP events around the contraction kernel); "
                               "host clock around the whole call; sides alternate, one process each"},
           "f16_this_tree_build_f16": f16,
           "f32_parent_build_of_widened_column" if a.parent_side == "f32" else "f16_parent_build_f16": f32,
           "final_assign_ratio_f32_over_f16" if a.parent_side == "f32" else "final_assign_ratio_parent_over_this_tree":
               round(f32["final_assign"]["median_ms"] / f16["final_assign"]["median_ms"], 4),
           "parent_final_assign_range_ms": round(parent_range, 3),
           "f16_final_assign_not_slower_beyond_parent_range": f16["final_assign"]["median_ms"] <= f32["final_assign"]["median_ms"] + parent_range,
           "verbose_exact_share": lines, "blobs_identical": True}
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
