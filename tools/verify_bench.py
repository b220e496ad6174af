#!/usr/bin/env python3
"""The database check measured at BASELINE C2 (1e8 x 13-byte keys); writes
profiles/verify/*.json (DESIGN.md quotes them).  Not part of bench.py.

  --resident  the fused bsdb_dev_verify_fixed against what the library could do
              before it with the same resident inputs: hash_fixed -> lookup
              (check) -> a torch gather-and-compare of the slots.  The two
              alternate in one process, HIP events, median and min-max.
  --kv        bsdb_kv_verify_index beside bsdb_kv_build_index on the same
              kv.db files (48-byte records, 8 partitions), wall clock.

python tools/verify_bench.py [--resident] [--kv] [--n N] [--reps R] [--out-dir D]"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "all_ms": ms}


def resident(ctx, n, reps):
    import torch
    base, stride = 0, 48  # the records of one compact data file with 48-byte records
    keys = ctx.gen_keys13(0, n)
    index = torch.zeros(n, dtype=torch.int64, device="cuda")
    E, values, sigbits, passes = ctx.mph_build_index_passes(keys, 13, n, 4, addr_base=base, addr_stride=stride,
                                                            index=index)
    # the composition's expected slots (big-endian addresses), made before the clock
    addr = torch.arange(n, dtype=torch.int64, device="cuda") * stride + base
    want = addr.view(torch.uint8).view(n, 8).flip(1).contiguous().view(torch.int64).view(n)
    del addr
    sig = torch.empty((n, 2), dtype=torch.int64, device="cuda")
    rank = torch.empty(n, dtype=torch.int64, device="cuda")
    out = ctx.verify_out("cuda")

    def fused():
        out.zero_()
        out[5] = -1
        ctx.verify_fixed(keys, 13, n, E, values, index, width=4, sigbits=sigbits, addr_base=base,
                         addr_stride=stride, out=out)

    def composed():
        ctx.hash_fixed(keys, 13, out=sig)
        ctx.lookup(sig, n, E, values, 4, sigbits, check=True, out=rank)
        rejected = (rank < 0).sum()
        wrong = (index[rank.clamp(min=0)] != want).sum()
        return int(rejected), int(wrong)

    def timed(f):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = f()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), r

    fused(), composed()  # warm-up of both
    tf, tc = [], []
    for _ in range(reps):
        t, _ = timed(fused)
        tf.append(t)
        t, r = timed(composed)
        tc.append(t)
    got = [int(x) & (2**64 - 1) for x in out.cpu().tolist()]
    clean = got[:6] == [n, 0, n, 0, 0, 2**64 - 1] and r == (0, 0)
    f, c = spread(tf), spread(tc)
    return {"leg": "C2 resident", "n_keys": n, "checksum_bits": 4, "reps": reps, "build_passes": passes,
            "fused": f, "composition": c, "fused_keys_per_s": n / (f["median_ms"] * 1e-3),
            "composition_keys_per_s": n / (c["median_ms"] * 1e-3),
            "fused_over_composition": f["median_ms"] / c["median_ms"], "both_clean": clean,
            "what": "bsdb_dev_verify_fixed (addresses by stride) vs bsdb_dev_hash_fixed -> bsdb_dev_lookup(check) -> "
                    "torch index[rank] != expected big-endian address (expected slots precomputed), alternating, "
                    "HIP events"}


def kv(ctx, n, reps, partitions):
    import bench
    import torch
    need = 48 * n + 8 * n
    d, _ = bench._roomiest_dir(need)
    if d is None:
        return {"leg": "C2 kv.db", "skipped": f"no directory with {need / 1e9:.1f} GB free"}
    tmp = tempfile.mkdtemp(prefix="bsdb_vfy_", dir=d)
    try:
        base = os.path.join(tmp, "kv.db")
        per = -(-n // partitions)
        for p in range(partitions):
            lo, hi = p * per, min(n, (p + 1) * per)
            with open(f"{base}.{p}", "wb") as f:
                for c0 in range(lo, hi, 1 << 24):
                    k = min(1 << 24, hi - c0)
                    rec = torch.empty((k, 48), dtype=torch.uint8, device="cuda")
                    rec[:, 0] = 13
                    rec[:, 1] = 0
                    rec[:, 2] = 32
                    rec[:, 3:16] = ctx.gen_keys13(c0, k).view(k, 13)
                    rec[:, 16:] = torch.randint(0, 256, (k, 32), dtype=torch.uint8, device="cuda")
                    rec.cpu().numpy().tofile(f)
                    del rec
        torch.cuda.empty_cache()
        ip, ap = os.path.join(tmp, "index.db"), os.path.join(tmp, "index_a.db")
        tb, tv, rep = [], [], None
        for _ in range(reps):
            t0 = time.perf_counter()
            mph = ctx.kv_build_index(base, partitions, 4, ip, ap)
            tb.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            rep = mph.verify_kv(base, partitions, ip, ap)
            tv.append((time.perf_counter() - t0) * 1e3)
            mph.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    b, v = spread(tb), spread(tv)
    return {"leg": "C2 kv.db", "n_keys": n, "partitions": partitions, "kv_db_bytes": 48 * n, "reps": reps,
            "host_cpus": bench.usable_cpus(), "kv_build_index": b, "kv_verify_index": v,
            "verify_keys_per_s": n / (v["median_ms"] * 1e-3), "build_keys_per_s": n / (b["median_ms"] * 1e-3),
            "report": rep, "what": "bsdb_kv_build_index then bsdb_kv_verify_index on the same files, wall clock"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resident", action="store_true")
    ap.add_argument("--kv", action="store_true")
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kv-reps", type=int, default=2)
    ap.add_argument("--parts", type=int, default=8)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "verify"))
    args = ap.parse_args()
    from bsdb_amd import Context
    os.makedirs(args.out_dir, exist_ok=True)
    ctx = Context(0)
    for name, on, run in (("c2_resident", args.resident, lambda: resident(ctx, args.n, args.reps)),
                          ("c2_kv", args.kv, lambda: kv(ctx, args.n, args.kv_reps, args.parts))):
        if not on:
            continue
        res = run()
        print(json.dumps(res), flush=True)
        with open(os.path.join(args.out_dir, name + ".json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
