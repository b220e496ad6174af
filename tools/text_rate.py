#!/usr/bin/env python3
"""Measures the text front end (bsdb_text_build and its kernels) on the C2
shape: lines of a 13-byte key, a space and a value of 8..64 bytes, ended by
"\\n".  Writes one JSON file (default profiles/text/c2.json) with the library's
sha256.  Medians of 5 timed runs after 2 warm-ups, all values kept.

  (a) kernels     device-event time of split + pack per chunk, beside a
                  device-to-device copy of the same chunk bytes (the floor for
                  touching the text once), and their ratio
  (b) end to end  wall clock of bsdb_text_build beside bsdb_kv_build_index over
                  the kv.db files it just wrote (existing code on the same
                  records that does strictly less); the difference is the cost
                  of the new front end
  (c) the solve   split + pack kernel time of the whole set beside the GOV
                  build (hash + solve, device events) of the same keys

  --blocked       a leg of its own (default output profiles/text/
                  c2_blocked.json): per chunk, the device-event time of split +
                  blocked pack (bsdb_dev_text_pack_blocked, --block-size) beside
                  split + compact pack of the same chunk in the same run, their
                  ratio, and the blocked image's bytes against the compact
                  image's.  With --once every leg runs once and nothing is
                  written: the form to put under a kernel trace.

The lines are generated on the host.  --lines defaults to 1e7: generating 1e8
lines (5 GB of text) on the host and building them seven times takes minutes;
pass --lines 100000000 for the full C2 size.
"""
import argparse
import hashlib
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM, RUNS = 2, 5
CHUNK = 256 << 20


def make_text(n: int, seed: int = 1) -> np.ndarray:
    """n lines "<13 digits> <8..64 letters>\\n" as one uint8 array."""
    rng = np.random.default_rng(seed)
    vlen = rng.integers(8, 65, n, dtype=np.int64)
    llen = 13 + 1 + vlen + 1
    off = np.concatenate([[0], np.cumsum(llen)])
    buf = rng.integers(97, 123, int(off[-1]), dtype=np.uint8)
    ids = np.arange(n, dtype=np.int64) * 7919 + 1_000_000_007   # distinct 13-digit keys
    for d in range(13):
        buf[off[:-1] + d] = 48 + (ids // 10 ** (12 - d)) % 10
    buf[off[:-1] + 13] = 32
    buf[off[1:] - 1] = 10
    return buf


def timed(fn):
    vals = []
    for i in range(WARM + RUNS):
        t0 = time.perf_counter()
        r = fn()
        dt = r if isinstance(r, float) else time.perf_counter() - t0
        if i >= WARM:
            vals.append(dt)
    return {"median": statistics.median(vals), "values": vals}


def blocked_leg(ctx, torch, text, cuts, a) -> dict:
    """Split + pack per chunk, compact and blocked, device events around each pair of calls."""
    from bsdb_amd.native import text_image_max

    def ev_ms(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) / 1e3

    chunks = []
    for lo, hi in cuts:
        n = hi - lo
        t = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
        t[:n] = torch.from_numpy(text[lo:hi]).cuda()
        desc = torch.empty((4, n // 4 + 1), dtype=torch.int32, device="cuda")
        image = torch.empty(text_image_max(n, a.partitions, 1, a.block_size), dtype=torch.uint8, device="cuda")
        blob = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
        state = {}

        def leg(block_size):
            _, rep = ctx.text_split(t, " ", nbytes=n, desc=desc)
            k = int(rep[1])
            out = ctx.text_pack(t, desc, k, a.partitions, [0] * a.partitions, nbytes=n, image=image, blob=blob,
                                block_size=block_size)
            state[block_size] = (k, sum(out["run_bytes"]))

        if a.once:
            leg(None)
            leg(a.block_size)
            torch.cuda.synchronize()
            continue
        compact = timed(lambda: ev_ms(lambda: leg(None)))
        blocked = timed(lambda: ev_ms(lambda: leg(a.block_size)))
        chunks.append({"bytes": n, "records": state[None][0], "compact_split_pack_s": compact,
                       "blocked_split_pack_s": blocked, "ratio": blocked["median"] / compact["median"],
                       "compact_image_bytes": state[None][1], "blocked_image_bytes": state[a.block_size][1],
                       "image_ratio": state[a.block_size][1] / state[None][1]})
        del t, desc, image, blob
    if a.once:
        return {}
    tot_c = sum(c["compact_split_pack_s"]["median"] for c in chunks)
    tot_b = sum(c["blocked_split_pack_s"]["median"] for c in chunks)
    return {"block_size": a.block_size, "chunks": chunks, "compact_total_s": tot_c, "blocked_total_s": tot_b,
            "ratio": tot_b / tot_c,
            "image_ratio": sum(c["blocked_image_bytes"] for c in chunks) / sum(c["compact_image_bytes"] for c in chunks)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lines", type=int, default=10_000_000)
    ap.add_argument("--partitions", type=int, default=8)
    ap.add_argument("--out", default=None, help="default profiles/text/c2.json, with --blocked c2_blocked.json")
    ap.add_argument("--blocked", action="store_true", help="only the blocked leg beside the compact one")
    ap.add_argument("--block-size", type=int, default=4096)
    ap.add_argument("--once", action="store_true", help="with --blocked: every leg once, nothing written")
    ap.add_argument("--tmp", default=None, help="directory for the text and the database (default: a temporary one)")
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "text", "c2_blocked.json" if a.blocked else "c2.json")
    import torch
    from bsdb_amd import Context
    from bsdb_amd.native import LIB_PATH, TEXT_FIELDS

    tmp = a.tmp or tempfile.mkdtemp(prefix="text_rate_")
    os.makedirs(tmp, exist_ok=True)
    t0 = time.perf_counter()
    text = make_text(a.lines)
    path = os.path.join(tmp, "c2.txt")
    text.tofile(path)
    gen_s = time.perf_counter() - t0
    res = {"shape": "C2: 13-byte key, space, 8..64-byte value, \\n", "lines": a.lines, "text_bytes": int(text.size),
           "partitions": a.partitions, "warmups": WARM, "runs": RUNS, "host_generation_s": gen_s,
           "library_sha256": hashlib.sha256(open(LIB_PATH, "rb").read()).hexdigest()}
    # the chunks bsdb_text_build would make: cut after the last "\n" of each 256 MiB
    cuts, lo = [], 0
    while lo < text.size:
        hi = min(text.size, lo + CHUNK)
        if hi < text.size:
            hi = lo + int(np.flatnonzero(text[lo:hi] == 10)[-1]) + 1
        cuts.append((lo, hi))
        lo = hi
    if a.blocked:
        with Context(0) as ctx:
            res["blocked"] = blocked_leg(ctx, torch, text, cuts, a)
        if not a.tmp:
            shutil.rmtree(tmp, ignore_errors=True)
        if not a.once:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
            print(json.dumps({"lines": a.lines, "text_bytes": res["text_bytes"], "blocked_over_compact": res["blocked"]["ratio"],
                              "compact_s": res["blocked"]["compact_total_s"], "blocked_s": res["blocked"]["blocked_total_s"],
                              "image_ratio": res["blocked"]["image_ratio"]}))
        return
    with Context(0) as ctx:
        def ev_ms(fn):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            e.synchronize()
            return s.elapsed_time(e) / 1e3

        # (a) split + pack per chunk beside a device-to-device copy of the chunk
        chunks, keys_blob = [], []
        for lo, hi in cuts:
            n = hi - lo
            t = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
            t[:n] = torch.from_numpy(text[lo:hi]).cuda()
            dst = torch.empty_like(t)
            desc = torch.empty((4, n // 4 + 1), dtype=torch.int32, device="cuda")
            image = torch.empty(n + n // 2 + 16, dtype=torch.uint8, device="cuda")
            blob = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
            state = {}

            def split_pack():
                _, rep = ctx.text_split(t, " ", nbytes=n, desc=desc)
                k = int(rep[1])
                state["k"] = k
                state["out"] = ctx.text_pack(t, desc, k, a.partitions, [0] * a.partitions, nbytes=n, image=image, blob=blob)

            sp = timed(lambda: ev_ms(split_pack))
            cp = timed(lambda: ev_ms(lambda: dst.copy_(t)))
            # the two halves on their own (each with the host round trips it makes)
            so = timed(lambda: ev_ms(lambda: ctx.text_split(t, " ", nbytes=n, desc=desc)))
            po = timed(lambda: ev_ms(lambda: ctx.text_pack(t, desc, state["k"], a.partitions, [0] * a.partitions, nbytes=n,
                                                           image=image, blob=blob)))
            chunks.append({"bytes": n, "records": state["k"], "split_pack_s": sp, "d2d_copy_s": cp, "split_s": so, "pack_s": po,
                           "ratio": sp["median"] / cp["median"], "text_GBps": n / sp["median"] / 1e9})
            keys_blob.append(state["out"]["blob"].clone())
            del t, dst, desc, image, blob, state
        res["kernels"] = {"chunks": chunks, "split_pack_total_s": sum(c["split_pack_s"]["median"] for c in chunks),
                          "d2d_copy_total_s": sum(c["d2d_copy_s"]["median"] for c in chunks)}
        res["kernels"]["ratio"] = res["kernels"]["split_pack_total_s"] / res["kernels"]["d2d_copy_total_s"]

        # (c) the GOV build of the same keys: hash + solve, device events
        keys = torch.cat(keys_blob + [torch.zeros(16, dtype=torch.uint8, device="cuda")])
        del keys_blob
        nk = (keys.numel() - 16) // 13
        assert nk == a.lines

        def gov():
            sig = ctx.hash_fixed(keys[: 13 * nk], 13)
            ctx.gov_build(sig, 4)

        res["gov_build_s"] = timed(lambda: ev_ms(gov))
        res["split_pack_over_gov_build"] = res["kernels"]["split_pack_total_s"] / res["gov_build_s"]["median"]
        del keys
        torch.cuda.empty_cache()

        # (b) bsdb_text_build beside bsdb_kv_build_index over the files it wrote
        db = os.path.join(tmp, "db")
        os.makedirs(db, exist_ok=True)
        kv, ix, ia = (os.path.join(db, f) for f in ("kv.db", "index.db", "index_a.db"))
        last = {}

        def text_build():
            mph, rep = ctx.text_build([path], " ", kv, a.partitions, 4, ix, ia)
            mph.close()
            last.update(rep)

        def kv_build():
            ctx.kv_build_index(kv, a.partitions, 4, ix, ia).close()

        tb = timed(text_build)
        kb = timed(kv_build)
        assert last["records"] == a.lines, last
        res["end_to_end"] = {"text_build_s": tb, "kv_build_index_s": kb, "front_end_cost_s": tb["median"] - kb["median"],
                             "text_build_Mrecords_per_s": a.lines / tb["median"] / 1e6,
                             "report": {k: last[k] for k in TEXT_FIELDS}}
    if not a.tmp:
        shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("lines", "text_bytes", "split_pack_over_gov_build")} |
                     {"kernel_ratio_to_copy": res["kernels"]["ratio"], "text_build_s": tb["median"],
                      "kv_build_index_s": kb["median"]}))


if __name__ == "__main__":
    main()
