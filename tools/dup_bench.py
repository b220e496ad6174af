#!/usr/bin/env python3
"""The duplicate finder measured at BASELINE C2 (1e8 resident 13-byte keys);
writes profiles/dup/c2.json (DESIGN.md §3.5 quotes it).  Not part of bench.py.

In one process, with one library: bsdb_dev_find_duplicates_fixed on the clean
key set and on the same set with 100 planted pairs (wall clock around the
synchronous call, median and min-max), then bench.py's gpu_c2 leg
(full_build_gpu: hash -> GOV build with ranks -> index scatter) on the same
keys.  The finder does the build's grouping and none of its solve, so its time
on the clean set must lie below the build's ("finder_below_build").

python tools/dup_bench.py [--n N] [--reps R] [--out FILE]"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "all_ms": ms}


def timed_find(ctx, keys, n, reps):
    import torch
    ms, rep = [], None
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rep = ctx.find_duplicates_fixed(keys, 13, n=n, cap=1 << 16)
        ms.append((time.perf_counter() - t0) * 1e3)
    return spread(ms[1:]), rep  # (the first call grows the workspace)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--planted", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dup", "c2.json"))
    args = ap.parse_args()
    import torch
    import bench
    from bsdb_amd import Context
    from bsdb_amd.native import LIB_PATH
    n = args.n
    ctx = Context(0)
    keys = ctx.gen_keys13(0, n)
    clean_t, clean = timed_find(ctx, keys, n, args.reps)
    g = torch.Generator().manual_seed(1)
    perm = torch.randperm(n, generator=g)[: 2 * args.planted].cuda()
    src, dst = perm[: args.planted], perm[args.planted:]
    rows = keys.view(n, 13)
    saved = rows[dst].clone()
    rows[dst] = rows[src]
    planted_t, planted = timed_find(ctx, keys, n, args.reps)
    want = sorted((min(a, b), max(a, b)) for a, b in zip(src.cpu().tolist(), dst.cpu().tolist()))
    planted_ok = planted["found"] == args.planted and planted["pairs"].tolist() == [list(p) for p in want] and \
        not planted["kinds"].any()
    rows[dst] = saved
    del keys, rows, saved
    ctx.release_workspace()
    torch.cuda.empty_cache()
    build = bench.full_build_gpu(ctx, n, 4, max(2, args.reps // 2))
    ctx.close()
    res = {"leg": "C2 resident", "n_keys": n, "reps": args.reps,
           "library_sha256": hashlib.sha256(open(LIB_PATH, "rb").read()).hexdigest(),
           "finder_clean": clean_t, "finder_planted": planted_t, "planted_pairs": args.planted,
           "clean_found": clean["found"], "clean_keys": clean["keys"], "planted_found": planted["found"],
           "planted_pairs_exact": bool(planted_ok), "gpu_c2_build": build,
           "finder_clean_keys_per_s": n / (clean_t["median_ms"] * 1e-3),
           "finder_below_build": clean_t["median_ms"] < build["ms"],
           "what": "bsdb_dev_find_duplicates_fixed (passes = 0, cap 65 536), wall clock around the synchronous call, "
                   "after one warm call; then bench.py full_build_gpu on the same generated keys, HIP events, median"}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
